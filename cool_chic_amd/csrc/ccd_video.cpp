// ccd_video.cpp - the conveniences of include/ccd.h over a batch: one cool-chic, one inter frame, a whole video.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <new>

#include "ccd_host.hpp"
#include "ccd_kernels.hpp"

using namespace ccd;

extern "C" {

// -------------------------------------------------------------------------------------------------
// One-shot conveniences
// -------------------------------------------------------------------------------------------------
int ccd_decode_coolchic(const uint8_t* cc_header, size_t n_hdr, const uint8_t* bytes_nn, size_t n_nn,
                        const uint8_t* bytes_latent, size_t n_lat, int device, void* stream, float* out,
                        int out_on_device) {
    if (!out) return CCD_ERR_ARG;
    if (!bytes_latent) return CCD_ERR_ARG;  // coolchic.py:46-51
    ccd_batch* b = nullptr;
    int rc = ccd_batch_create(device, &b);
    if (rc < 0) return rc;
    rc = ccd_batch_add(b, cc_header, n_hdr, bytes_nn, n_nn, bytes_latent, n_lat, 0, 0);
    if (rc >= 0) rc = ccd_batch_run(b, stream);
    if (rc >= 0) rc = ccd_batch_wait(b, stream);
    if (rc >= 0) {
        const ccd_cc_header& h = b->slots[0]->hdr;
        const size_t bytes = static_cast<size_t>(h.out_channels) * h.img_size[0] * h.img_size[1] * 4;
        hipStream_t st = static_cast<hipStream_t>(stream);
        if (hipMemcpyAsync(out, b->slots[0]->d_out, bytes, out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            rc = CCD_ERR_HIP;
    }
    ccd_batch_destroy(b);
    return rc;
}

// ccd_decode_video hands out every plane of every frame inside ONE pinned host block (filled by one copy); its handle rides
// in a hidden ccd_frame behind the last one.
void ccd_video_free(ccd_video* v) {
    if (!v || !v->frames) return;
    Block* blk = reinterpret_cast<Block*>(v->frames[v->n_frames].plane[0]);
    if (blk) { blk->drop(); delete blk; }
    std::free(v->frames);
    v->frames = nullptr; v->n_frames = 0;
}

// decode.py:156-206 for one P / B frame on `st`, no allocation, no wait: tmp = 9 h w floats (two references and the result as
// 4:4:4 f32 planes).
static int inter_reconstruct_on(hipStream_t st, float* tmp, int frame_type, int h, int w, int bitdepth, int frame_data_type,
                                const float* residue, const float* motion, const void* const* ref0_planes, const void* const* ref1_planes,
                                const int32_t* global_flow, int warp_filter_size, void* const* out_planes, const void* coef = nullptr) {
    float* ref0 = tmp;
    float* ref1 = tmp + static_cast<size_t>(3) * h * w;
    float* out = tmp + static_cast<size_t>(6) * h * w;
    int gf[4] = {global_flow[0], global_flow[1], frame_type == 2 ? global_flow[2] : 0, frame_type == 2 ? global_flow[3] : 0};
    if (launch_planes_to_444(ref0_planes[0], ref0_planes[1], ref0_planes[2], ref0, h, w, bitdepth, frame_data_type, st) != hipSuccess) return CCD_ERR_HIP;
    if (frame_type == 2 &&
        launch_planes_to_444(ref1_planes[0], ref1_planes[1], ref1_planes[2], ref1, h, w, bitdepth, frame_data_type, st) != hipSuccess) return CCD_ERR_HIP;
    if (coef) {  // the sinc-8 coefficients were computed ahead of the references (ccd_decode_video): gather only
        if (launch_inter_apply8(frame_type, h, w, gf, residue, motion, ref0, frame_type == 2 ? ref1 : ref0, coef, out, st) != hipSuccess) return CCD_ERR_HIP;
    } else if (launch_inter_recon(frame_type, h, w, warp_filter_size, gf, residue, motion, ref0, frame_type == 2 ? ref1 : ref0, out, st) != hipSuccess) return CCD_ERR_HIP;
    if (launch_planes(out, out_planes[0], out_planes[1], out_planes[2], h, w, bitdepth, frame_data_type, st) != hipSuccess) return CCD_ERR_HIP;
    return CCD_OK;
}

int ccd_inter_reconstruct(int device, void* stream, int frame_type, int h, int w, int bitdepth, int frame_data_type,
                          const float* residue, const float* motion, const void* const* ref0_planes,
                          const void* const* ref1_planes, const int32_t* global_flow, int warp_filter_size,
                          void* const* out_planes) {
    if ((frame_type != 1 && frame_type != 2) || !residue || !motion || !ref0_planes || !global_flow || !out_planes ||
        (frame_type == 2 && !ref1_planes) || h <= 0 || w <= 0 || bitdepth < 8 || bitdepth > 16)
        return CCD_ERR_ARG;
    if (!warp_filter_ok(warp_filter_size)) return CCD_ERR_VALUE;
    if (frame_data_type < 0 || frame_data_type > 3 || !yuv420_sides_ok(frame_data_type, h, w)) return CCD_ERR_VALUE;
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    Block tmp;
    if (!tmp.get(device, BlockPool::kDevice, static_cast<size_t>(9) * h * w * sizeof(float))) return CCD_ERR_NOMEM;
    int rc = inter_reconstruct_on(st, tmp.as<float>(), frame_type, h, w, bitdepth, frame_data_type, residue, motion, ref0_planes, ref1_planes,
                                  global_flow, warp_filter_size, out_planes);
    if (hipStreamSynchronize(st) != hipSuccess) rc = CCD_ERR_HIP;
    tmp.drop();
    return rc;
}

}  // extern "C"

// ---- ccd_decode_video in steps over one state.  Every cool-chic of every frame is independent: all of them go into ONE batch and
// decode concurrently; the cheap reconstruction then walks the frames in coding order (decode.py:67-81).
namespace {
struct DevFrame { void* plane[3] = {nullptr, nullptr, nullptr}; int h = 0, w = 0, ch = 0, cw = 0, bitdepth = 0, fdt = 0; bool seen = false; Block own; };

// What one call holds, and its release (the destructor: every return reaches it).
struct VideoDecode {
    const uint8_t* bs; size_t n; int device; ccd_video* v;
    // CCD_VIDEO_TIMING=1: host wall clock of the call's phases on stderr (tools/prof_gop.py)
    const bool timing = std::getenv("CCD_VIDEO_TIMING") != nullptr;
    const std::chrono::steady_clock::time_point t_start = std::chrono::steady_clock::now();
    int n_frames = 0;
    ccd_batch* b = nullptr;
    std::vector<ccd_frame_header> fhs;  // by coding index, as first_slot: the frame's first cool-chic in the batch
    std::vector<int> first_slot;
    std::vector<Block> coef;            // warp coefficients computed ahead of the references (by coding index), and the event behind each
    std::vector<hipEvent_t> coef_done;
    std::vector<DevFrame> dev;          // by display index: device planes of every decoded frame are kept for references
    Block tmp;                          // two references and the result as 4:4:4 f32 planes, reused by every inter frame (one stream: ordered)
    size_t tmp_elems = 0;
    Block wide;                         // every plane of every frame as u16: staging of the host block, same layout
    Block* host = nullptr;              // the pinned block ccd_video hands out; the caller's once handed_out
    bool handed_out = false;
    std::vector<size_t> off;            // [display index][plane] -> offset in wide / host
    size_t total = 0;
    hipStream_t copy_st = nullptr;
    hipEvent_t frame_done = nullptr;

    void mark(const char* what) const {
        if (timing) std::fprintf(stderr, "[ccd_decode_video] %-28s %8.2f ms\n", what,
                                 std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count());
    }
    ~VideoDecode() {
        if (!b) return;  // no batch: nothing was enqueued or taken from the pool
        if (!handed_out) {
            if (host) { host->drop(); delete host; }
            std::free(v->frames);
            v->frames = nullptr; v->n_frames = 0;
        }
        (void)hipStreamSynchronize(copy_st);
        if (frame_done) (void)hipEventDestroy(frame_done);
        for (hipEvent_t e : coef_done) if (e) (void)hipEventDestroy(e);
        for (auto& c : coef) c.drop();
        (void)hipStreamSynchronize(nullptr);  // nothing may still read the blocks that go back to the pool
        for (auto& d : dev) d.own.drop();
        tmp.drop(); wide.drop();
        ccd_batch_destroy(b);
        mark("batch destroyed");
    }
};

// the frame headers behind the video header (`pos`), every cool-chic into the batch
int video_parse(VideoDecode& s, const ccd_video_header& vh, size_t pos) {
    // decode.py:52-75: the coding order and every frame's references come from the VIDEO header's coding structure
    std::vector<CodedFrame> cs;
    int rc = coding_structure(vh, cs);
    for (int f = 0; f < s.n_frames && rc >= 0; ++f) {
        ccd_frame_header& fh = s.fhs[f];
        const int used = read_frame_header(s.bs + pos, s.n - pos, &fh);
        if (used < 0) return used;
        // decode.py:67-75 takes the display index and the references of the frame at this coding index from the STRUCTURE and
        // never reads those fields of the frame header; the header's frame_type decides how many cool-chics follow and how the
        // frame is reconstructed (decode.py:119-128, 156-189), whatever the structure calls the frame: a header "I" at a P / B
        // position decodes as plain intra (decode_frame ignores reference_frames), a header "P" at a B position predicts from
        // the structure's first reference only (apply_global_translation zips references with flows).  Rejected is only what
        // the reference raises on: a header type that needs MORE references than the structure gives (raw_references[0] /
        // shifted_ref[1]: IndexError)
        const CodedFrame& want = cs[f];
        if (fh.frame_type > want.n_refs) return CCD_ERR_VALUE;  // I / P / B = 0 / 1 / 2 = references needed
        fh.display_index = want.display_order;
        fh.n_refs = fh.frame_type;
        for (int k = 0; k < fh.n_refs; ++k) fh.index_references[k] = want.refs[k];
        pos += static_cast<size_t>(used);
        s.first_slot[f] = ccd_batch_size(s.b);
        const int n_cc = fh.frame_type == 0 ? 1 : 2;  // residue (+ motion), decode.py:126-128
        for (int c = 0; c < n_cc && rc >= 0; ++c) {
            ccd_cc_header ch;
            const int used_cc = read_cc_header(s.bs + pos, s.n - pos, &ch);
            if (used_cc < 0) return used_cc;
            const uint8_t* hdr = s.bs + pos;
            pos += static_cast<size_t>(used_cc);
            if (pos + static_cast<size_t>(ch.nn_n_bytes) + static_cast<size_t>(ch.n_bytes_latent) > s.n) return CCD_ERR_TRUNCATED;
            const bool intra = fh.frame_type == 0;
            rc = ccd_batch_add(s.b, hdr, static_cast<size_t>(used_cc), s.bs + pos, ch.nn_n_bytes, s.bs + pos + ch.nn_n_bytes, ch.n_bytes_latent,
                               intra ? fh.bitdepth : 0, fh.frame_data_type);
            pos += static_cast<size_t>(ch.nn_n_bytes) + static_cast<size_t>(ch.n_bytes_latent);
        }
    }
    return rc;
}

// ---- r06, OFF by default (CCD_VIDEO_COEF_MB = scratch budget in MB): the warp coefficients of the inter frames ahead of their
// references.  The cool-chics of a hierarchical GOP's B frames are decoded at about half of the I frames' chains, and every
// reconstruction then waits for the I frames; a frame's sinc coefficients (f64 sin / cos) only need its flows.  With a budget they
// are computed on the copy stream as soon as the launch of the frame's motion cool-chic is done (ccd_batch::lg_done), 64 B per pixel
// and reference, and the reconstruction only gathers.  Same bits either way (test_video_warp_coefficients_ahead_of_the_references).
// Measured on the 33-frame 1080p GOP (profiles/r06/gop_timing_coefficients_ahead.txt): 174.0 against 175.1 ms for 8.2 GB of
// scratch - the gather of the 2 x 64 x 3 taps is 0.26 of the 0.34 ms a frame takes, the f64 work only the rest.  Not worth the
// memory by default.
int video_coefficients_ahead(VideoDecode& s) {
    ccd_batch* b = s.b;
    if (!b->lg_valid) return CCD_OK;
    size_t budget = 0;
    if (const char* e = std::getenv("CCD_VIDEO_COEF_MB")) budget = static_cast<size_t>(std::max(0, std::atoi(e)));
    budget <<= 20;
    size_t spent = 0;
    for (int f = 0; f < s.n_frames; ++f) {
        const ccd_frame_header& fh = s.fhs[f];
        if (fh.frame_type == 0 || fh.warp_filter_size != 8) continue;
        const Slot& s0 = *b->slots[s.first_slot[f]];
        const Slot& s1 = *b->slots[s.first_slot[f] + 1];
        const int h = s0.hdr.img_size[0], w = s0.hdr.img_size[1];
        if (s1.hdr.out_channels < inter_channels(fh.frame_type, 1) || s1.hdr.img_size[0] != h || s1.hdr.img_size[1] != w) continue;  // (rejected by video_reconstruct_frame)
        if (s1.lg < 0 || s1.fl != s1.lg || static_cast<size_t>(s1.lg) >= b->lg_done.size() || !b->lg_done[s1.lg] || !s1.use_fused_dec || s1.cr)
            continue;  // its output is only complete behind the join
        const size_t bytes = inter_coef_bytes(fh.frame_type, h, w);
        if (spent + bytes > budget) break;
        if (!s.coef[f].get(s.device, BlockPool::kDevice, bytes)) break;
        spent += bytes;
        if (hipStreamWaitEvent(b->up_stream, b->lg_done[s1.lg], 0) != hipSuccess ||
            launch_inter_coef8(fh.frame_type, h, w, s1.d_out, s.coef[f].p, b->up_stream) != hipSuccess ||
            hipEventCreateWithFlags(&s.coef_done[f], hipEventDisableTiming) != hipSuccess ||
            hipEventRecord(s.coef_done[f], b->up_stream) != hipSuccess) return CCD_ERR_HIP;
    }
    return CCD_OK;
}

// geometry of every frame is known from the headers: checked, and the host block and the u16 staging block laid out up front
int video_layout(VideoDecode& s) {
    const int n_frames = s.n_frames;
    for (int f = 0; f < n_frames; ++f) {  // sizes by display index
        const ccd_frame_header& fh = s.fhs[f];
        if (fh.display_index < 0 || fh.display_index >= n_frames) return CCD_ERR_VALUE;
        DevFrame& d = s.dev[fh.display_index];
        if (d.seen) return CCD_ERR_VALUE;  // two frames with one display index: the second would overwrite the first
        d.seen = true;
        const Slot& s0 = *s.b->slots[s.first_slot[f]];
        d.h = s0.hdr.img_size[0]; d.w = s0.hdr.img_size[1]; d.bitdepth = fh.bitdepth; d.fdt = fh.frame_data_type;
        if (!yuv420_sides_ok(fh.frame_data_type, d.h, d.w)) return CCD_ERR_VALUE;
        d.ch = fh.frame_data_type == 1 ? d.h / 2 : d.h; d.cw = fh.frame_data_type == 1 ? d.w / 2 : d.w;
    }
    // every display index must have been produced (a gap would leave a frame without planes)
    for (int i = 0; i < n_frames; ++i) if (!s.dev[i].seen) return CCD_ERR_VALUE;
    for (int i = 0; i < n_frames; ++i)
        for (int p = 0; p < 3; ++p) {
            s.off[static_cast<size_t>(i) * 3 + p] = s.total;
            s.total += ((p == 0 ? static_cast<size_t>(s.dev[i].h) * s.dev[i].w : static_cast<size_t>(s.dev[i].ch) * s.dev[i].cw) * 2 + 63) & ~size_t{63};
        }
    s.host = new (std::nothrow) Block();
    s.v->frames = static_cast<ccd_frame*>(std::calloc(static_cast<size_t>(n_frames) + 1, sizeof(ccd_frame)));
    if (!s.host || !s.v->frames || !s.wide.get(s.device, BlockPool::kDevice, std::max<size_t>(s.total, 64)) ||
        !s.host->get(s.device, BlockPool::kPinned, std::max<size_t>(s.total, 64)))
        return CCD_ERR_NOMEM;
    HIP_TRY(hipEventCreateWithFlags(&s.frame_done, hipEventDisableTiming));
    return CCD_OK;
}

// r06: a frame's planes start their way to the host (u16 widening + one device -> host copy per frame on the library's upload
// stream, behind an event) as soon as the frame is reconstructed, while the following frames are still being warped: the 200 MB of
// a 33-frame 1080p GOP used to cross PCIe after the last frame (3.6 ms of a 190 ms call, profiles/r06/gop_timing_before.txt).
// planes of display index di: widened to u16 and copied to the host on the copy stream, behind everything enqueued so far
int video_send_frame(VideoDecode& s, int di) {
    const DevFrame& d = s.dev[di];
    HIP_TRY(hipEventRecord(s.frame_done, nullptr));
    HIP_TRY(hipStreamWaitEvent(s.copy_st, s.frame_done, 0));
    for (int p = 0; p < 3; ++p) {
        const size_t px = p == 0 ? static_cast<size_t>(d.h) * d.w : static_cast<size_t>(d.ch) * d.cw;
        uint16_t* dst = reinterpret_cast<uint16_t*>(s.wide.as<char>() + s.off[static_cast<size_t>(di) * 3 + p]);
        const hipError_t e = d.bitdepth == 8 ? launch_widen_u8(static_cast<const uint8_t*>(d.plane[p]), dst, px, s.copy_st)
                                             : hipMemcpyAsync(dst, d.plane[p], px * 2, hipMemcpyDeviceToDevice, s.copy_st);
        if (e != hipSuccess) return CCD_ERR_HIP;
    }
    const size_t o0 = s.off[static_cast<size_t>(di) * 3], o1 = di + 1 < s.n_frames ? s.off[static_cast<size_t>(di + 1) * 3] : s.total;
    HIP_TRY(hipMemcpyAsync(s.host->as<char>() + o0, s.wide.as<char>() + o0, o1 - o0, hipMemcpyDeviceToHost, s.copy_st));
    return CCD_OK;
}

// the device planes of coding index f: an intra frame's are its cool-chic's, a P / B frame is reconstructed from its references
int video_reconstruct_frame(VideoDecode& s, int f) {
    const ccd_frame_header& fh = s.fhs[f];
    DevFrame& d = s.dev[fh.display_index];
    const Slot& s0 = *s.b->slots[s.first_slot[f]];
    if (fh.frame_type == 0) {
        if (s0.hdr.out_channels < 3) return CCD_ERR_VALUE;
        for (int p = 0; p < 3; ++p) d.plane[p] = s0.d_plane[p];
        return CCD_OK;
    }
    const Slot& s1 = *s.b->slots[s.first_slot[f] + 1];
    if (s0.hdr.out_channels < inter_channels(fh.frame_type, 0) || s1.hdr.out_channels < inter_channels(fh.frame_type, 1) ||
        s1.hdr.img_size[0] != d.h || s1.hdr.img_size[1] != d.w) return CCD_ERR_VALUE;
    if (!warp_filter_ok(fh.warp_filter_size)) return CCD_ERR_VALUE;
    const void* refs[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    for (int k = 0; k < fh.n_refs; ++k) {
        const int ri = fh.index_references[k];
        // a reference must be a decoded frame of the same geometry AND sample layout: its planes are read with this
        // frame's layout (a 4:2:0 reference has quarter-size chroma planes)
        if (ri < 0 || ri >= s.n_frames || !s.dev[ri].plane[0] || s.dev[ri].h != d.h || s.dev[ri].w != d.w || s.dev[ri].bitdepth != d.bitdepth ||
            s.dev[ri].fdt != d.fdt) return CCD_ERR_VALUE;
        for (int p = 0; p < 3; ++p) refs[k][p] = s.dev[ri].plane[p];
    }
    const size_t sb = d.bitdepth == 8 ? 1 : 2;
    const size_t luma = align256(static_cast<size_t>(d.h) * d.w * sb + 16);
    const size_t chroma = align256(static_cast<size_t>(d.ch) * d.cw * sb + 16);
    if (!d.own.get(s.device, BlockPool::kDevice, luma + 2 * chroma)) return CCD_ERR_NOMEM;
    d.plane[0] = d.own.as<char>(); d.plane[1] = d.own.as<char>() + luma; d.plane[2] = d.own.as<char>() + luma + chroma;
    const size_t need = static_cast<size_t>(9) * d.h * d.w;
    if (need > s.tmp_elems) {
        if (s.tmp.p) HIP_TRY(hipStreamSynchronize(nullptr));  // frames in flight still use the smaller one
        if (!s.tmp.get(s.device, BlockPool::kDevice, need * sizeof(float))) return CCD_ERR_NOMEM;
        s.tmp_elems = need;
    }
    if (s.coef_done[f]) HIP_TRY(hipStreamWaitEvent(nullptr, s.coef_done[f], 0));
    return inter_reconstruct_on(nullptr, s.tmp.as<float>(), fh.frame_type, d.h, d.w, d.bitdepth, d.fdt, s0.d_out, s1.d_out, refs[0],
                                fh.frame_type == 2 ? refs[1] : nullptr, fh.global_flow, fh.warp_filter_size, d.plane,
                                s.coef_done[f] ? s.coef[f].p : nullptr);
}

// ccd_video: every plane points into the host block, whose handle rides behind the last frame (ccd_video_free)
void video_hand_out(VideoDecode& s) {
    ccd_video* v = s.v;
    v->n_frames = s.n_frames;
    v->frames[s.n_frames].plane[0] = reinterpret_cast<uint16_t*>(s.host);
    s.handed_out = true;
    for (int f = 0; f < s.n_frames; ++f) {
        const int di = s.fhs[f].display_index;
        const DevFrame& d = s.dev[di];
        ccd_frame& fr = v->frames[di];
        fr.display_index = di; fr.frame_type = s.fhs[f].frame_type; fr.frame_data_type = d.fdt; fr.bitdepth = d.bitdepth;
        fr.h = d.h; fr.w = d.w; fr.ch = d.ch; fr.cw = d.cw;
        for (int p = 0; p < 3; ++p) fr.plane[p] = reinterpret_cast<uint16_t*>(s.host->as<char>() + s.off[static_cast<size_t>(di) * 3 + p]);
    }
}
}  // namespace

extern "C" int ccd_decode_video(const uint8_t* bs, size_t n, int device, ccd_video* v) {
    if (!bs || !v) return CCD_ERR_ARG;
    v->n_frames = 0; v->frames = nullptr;
    VideoDecode s{bs, n, device, v};
    std::unique_ptr<ccd_video_header> vh(new (std::nothrow) ccd_video_header());
    if (!vh) return CCD_ERR_NOMEM;
    const int used = read_video_header(bs, n, vh.get());
    if (used < 0) return used;
    const int n_frames = s.n_frames = vh->n_frames;
    int rc = ccd_batch_create(device, &s.b);
    if (rc < 0) return rc;
    s.copy_st = s.b->up_stream;
    s.fhs.resize(n_frames); s.first_slot.resize(n_frames); s.coef.resize(n_frames); s.coef_done.resize(n_frames);
    s.dev.resize(n_frames); s.off.resize(static_cast<size_t>(n_frames) * 3);
    rc = video_parse(s, *vh, static_cast<size_t>(used));
    s.mark("parsed + added");
    if (rc >= 0) rc = ccd_batch_run(s.b, nullptr);
    s.mark("launched");
    if (rc >= 0) rc = video_coefficients_ahead(s);
    if (rc >= 0) rc = ccd_batch_wait(s.b, nullptr);
    s.mark("cool-chics decoded");
    if (rc >= 0) rc = video_layout(s);
    for (int f = 0; f < n_frames && rc >= 0; ++f) {  // in coding order
        rc = video_reconstruct_frame(s, f);
        if (rc >= 0) rc = video_send_frame(s, s.fhs[f].display_index);
    }
    if (s.timing) { (void)hipStreamSynchronize(nullptr); s.mark("reconstructed"); }
    if (rc >= 0 && hipStreamSynchronize(s.copy_st) != hipSuccess) rc = CCD_ERR_HIP;
    s.mark("planes on the host");
    if (rc >= 0) video_hand_out(s);
    return rc < 0 ? rc : CCD_OK;
}
