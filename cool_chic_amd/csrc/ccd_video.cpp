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
    // 2 / 4 taps = grid_sample bilinear / bicubic, 6.. = sinc (warp.py:49-56); odd or < 2 fails the reference's asserts (warp.py:41-47)
    if (warp_filter_size < 2 || warp_filter_size > 16 || (warp_filter_size & 1)) return CCD_ERR_VALUE;
    // 4:2:0 needs even sizes (as in ccd_decode_video): planes_to_444_kernel reads chroma at (y >> 1, x >> 1), past an h/2 x w/2 plane
    if (frame_data_type < 0 || frame_data_type > 3 || (frame_data_type == 1 && ((h | w) & 1))) return CCD_ERR_VALUE;
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

int ccd_decode_video(const uint8_t* bs, size_t n, int device, ccd_video* v) {
    if (!bs || !v) return CCD_ERR_ARG;
    v->n_frames = 0; v->frames = nullptr;
    // CCD_VIDEO_TIMING=1: host wall clock of the call's phases on stderr (tools/prof_gop.py)
    const bool timing = std::getenv("CCD_VIDEO_TIMING") != nullptr;
    const auto t_start = std::chrono::steady_clock::now();
    auto mark = [&](const char* what) {
        if (timing) std::fprintf(stderr, "[ccd_decode_video] %-28s %8.2f ms\n", what,
                                 std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count());
    };
    std::unique_ptr<ccd_video_header> vh(new (std::nothrow) ccd_video_header());
    if (!vh) return CCD_ERR_NOMEM;
    int used = read_video_header(bs, n, vh.get());
    if (used < 0) return used;
    size_t pos = static_cast<size_t>(used);
    const int n_frames = vh->n_frames;
    ccd_batch* b = nullptr;
    int rc = ccd_batch_create(device, &b);
    if (rc < 0) return rc;
    // Every cool-chic of every frame is independent: all of them go into ONE batch and decode concurrently; the cheap
    // reconstruction then walks the frames in coding order (decode.py:67-81).
    std::vector<ccd_frame_header> fhs(n_frames);
    std::vector<int> first_slot(n_frames, 0);
    // decode.py:52-75: the coding order and every frame's references come from the VIDEO header's coding structure
    std::vector<CodedFrame> cs;
    rc = coding_structure(*vh, cs);
    for (int f = 0; f < n_frames && rc >= 0; ++f) {
        used = read_frame_header(bs + pos, n - pos, &fhs[f]);
        if (used < 0) { rc = used; break; }
        {
            // decode.py:67-75 takes the display index and the references of the frame at this coding index from the STRUCTURE and
            // never reads those fields of the frame header; the header's frame_type decides how many cool-chics follow and how the
            // frame is reconstructed (decode.py:119-128, 156-189), whatever the structure calls the frame: a header "I" at a P / B
            // position decodes as plain intra (decode_frame ignores reference_frames), a header "P" at a B position predicts from
            // the structure's first reference only (apply_global_translation zips references with flows).  Rejected is only what
            // the reference raises on: a header type that needs MORE references than the structure gives (raw_references[0] /
            // shifted_ref[1]: IndexError)
            const CodedFrame& want = cs[f];
            if (fhs[f].frame_type > want.n_refs) { rc = CCD_ERR_VALUE; break; }  // I / P / B = 0 / 1 / 2 = references needed
            fhs[f].display_index = want.display_order;
            fhs[f].n_refs = fhs[f].frame_type;
            for (int k = 0; k < fhs[f].n_refs; ++k) fhs[f].index_references[k] = want.refs[k];
        }
        pos += static_cast<size_t>(used);
        first_slot[f] = ccd_batch_size(b);
        const int n_cc = fhs[f].frame_type == 0 ? 1 : 2;  // residue (+ motion), decode.py:126-128
        for (int c = 0; c < n_cc && rc >= 0; ++c) {
            ccd_cc_header ch;
            used = read_cc_header(bs + pos, n - pos, &ch);
            if (used < 0) { rc = used; break; }
            const uint8_t* hdr = bs + pos;
            pos += static_cast<size_t>(used);
            if (pos + static_cast<size_t>(ch.nn_n_bytes) + static_cast<size_t>(ch.n_bytes_latent) > n) { rc = CCD_ERR_TRUNCATED; break; }
            const bool intra = fhs[f].frame_type == 0;
            rc = ccd_batch_add(b, hdr, static_cast<size_t>(used), bs + pos, ch.nn_n_bytes, bs + pos + ch.nn_n_bytes, ch.n_bytes_latent,
                               intra ? fhs[f].bitdepth : 0, fhs[f].frame_data_type);
            pos += static_cast<size_t>(ch.nn_n_bytes) + static_cast<size_t>(ch.n_bytes_latent);
        }
    }
    mark("parsed + added");
    if (rc >= 0) rc = ccd_batch_run(b, nullptr);
    mark("launched");
    // ---- r06, OFF by default (CCD_VIDEO_COEF_MB = scratch budget in MB): the warp coefficients of the inter frames ahead of their
    // references.  The cool-chics of a hierarchical GOP's B frames are decoded at about half of the I frames' chains, and every
    // reconstruction then waits for the I frames; a frame's sinc coefficients (f64 sin / cos) only need its flows.  With a budget they
    // are computed on the copy stream as soon as the launch of the frame's motion cool-chic is done (ccd_batch::lg_done), 64 B per pixel
    // and reference, and the reconstruction only gathers.  Same bits either way (test_video_warp_coefficients_ahead_of_the_references).
    // Measured on the 33-frame 1080p GOP (profiles/r06/gop_timing_coefficients_ahead.txt): 174.0 against 175.1 ms for 8.2 GB of
    // scratch - the gather of the 2 x 64 x 3 taps is 0.26 of the 0.34 ms a frame takes, the f64 work only the rest.  Not worth the
    // memory by default.
    std::vector<Block> coef(n_frames);
    std::vector<hipEvent_t> coef_done(n_frames, nullptr);
    if (rc >= 0 && b->lg_valid) {
        size_t budget = 0;
        if (const char* e = std::getenv("CCD_VIDEO_COEF_MB")) budget = static_cast<size_t>(std::max(0, std::atoi(e)));
        budget <<= 20;
        size_t spent = 0;
        for (int f = 0; f < n_frames; ++f) {
            const ccd_frame_header& fh = fhs[f];
            if (fh.frame_type == 0 || fh.warp_filter_size != 8) continue;
            const Slot& s0 = *b->slots[first_slot[f]];
            const Slot& s1 = *b->slots[first_slot[f] + 1];
            const int h = s0.hdr.img_size[0], w = s0.hdr.img_size[1];
            if (s1.hdr.out_channels < (fh.frame_type == 1 ? 2 : 4) || s1.hdr.img_size[0] != h || s1.hdr.img_size[1] != w) continue;  // (rejected below)
            if (s1.lg < 0 || s1.fl != s1.lg || static_cast<size_t>(s1.lg) >= b->lg_done.size() || !b->lg_done[s1.lg] || !s1.use_fused_dec || s1.cr)
                continue;  // its output is only complete behind the join
            const size_t bytes = inter_coef_bytes(fh.frame_type, h, w);
            if (spent + bytes > budget) break;
            if (!coef[f].get(device, BlockPool::kDevice, bytes)) break;
            spent += bytes;
            if (hipStreamWaitEvent(b->up_stream, b->lg_done[s1.lg], 0) != hipSuccess ||
                launch_inter_coef8(fh.frame_type, h, w, s1.d_out, coef[f].p, b->up_stream) != hipSuccess ||
                hipEventCreateWithFlags(&coef_done[f], hipEventDisableTiming) != hipSuccess ||
                hipEventRecord(coef_done[f], b->up_stream) != hipSuccess) { rc = CCD_ERR_HIP; break; }
        }
    }
    if (rc >= 0) rc = ccd_batch_wait(b, nullptr);
    mark("cool-chics decoded");
    // ---- frame reconstruction in coding order; device planes of every decoded frame are kept for references.  r06: a frame's
    // planes start their way to the host (u16 widening + one device -> host copy per frame on the library's upload stream, behind
    // an event) as soon as the frame is reconstructed, while the following frames are still being warped: the 200 MB of a 33-frame
    // 1080p GOP used to cross PCIe after the last frame (3.6 ms of a 190 ms call, profiles/r06/gop_timing_before.txt).
    struct DevFrame { void* plane[3] = {nullptr, nullptr, nullptr}; int h = 0, w = 0, ch = 0, cw = 0, bitdepth = 0, fdt = 0; bool seen = false; Block own; };
    std::vector<DevFrame> dev(n_frames);  // by display index
    Block tmp;  // two references and the result as 4:4:4 f32 planes, reused by every inter frame (one stream: ordered)
    size_t tmp_elems = 0;
    // geometry of every frame is known from the headers: the host block and the u16 staging block are laid out up front
    Block wide;
    Block* host = nullptr;
    std::vector<size_t> off(static_cast<size_t>(n_frames) * 3, 0);
    size_t total = 0;
    hipStream_t copy_st = b->up_stream;
    hipEvent_t frame_done = nullptr;
    if (rc >= 0) {
        for (int f = 0; f < n_frames && rc >= 0; ++f) {  // sizes by display index
            const ccd_frame_header& fh = fhs[f];
            if (fh.display_index < 0 || fh.display_index >= n_frames) { rc = CCD_ERR_VALUE; break; }
            DevFrame& d = dev[fh.display_index];
            if (d.seen) { rc = CCD_ERR_VALUE; break; }  // two frames with one display index: the second would overwrite the first
            d.seen = true;
            const Slot& s0 = *b->slots[first_slot[f]];
            d.h = s0.hdr.img_size[0]; d.w = s0.hdr.img_size[1]; d.bitdepth = fh.bitdepth; d.fdt = fh.frame_data_type;
            // 4:2:0 needs even sizes: F.avg_pool2d(2) drops the odd row / column and write_yuv's chroma planes are h/2 x w/2,
            // while the reference's 4:4:4 round trip of such a frame (yuv.py:303-316) no longer matches the luma size
            if (fh.frame_data_type == 1 && ((d.h | d.w) & 1)) { rc = CCD_ERR_VALUE; break; }
            d.ch = fh.frame_data_type == 1 ? d.h / 2 : d.h; d.cw = fh.frame_data_type == 1 ? d.w / 2 : d.w;
        }
        // every display index must have been produced (a gap would leave a frame without planes)
        for (int i = 0; i < n_frames && rc >= 0; ++i) if (!dev[i].seen) rc = CCD_ERR_VALUE;
    }
    if (rc >= 0) {
        for (int i = 0; i < n_frames; ++i)
            for (int p = 0; p < 3; ++p) {
                off[static_cast<size_t>(i) * 3 + p] = total;
                total += ((p == 0 ? static_cast<size_t>(dev[i].h) * dev[i].w : static_cast<size_t>(dev[i].ch) * dev[i].cw) * 2 + 63) & ~size_t{63};
            }
        host = new (std::nothrow) Block();
        v->frames = static_cast<ccd_frame*>(std::calloc(static_cast<size_t>(n_frames) + 1, sizeof(ccd_frame)));
        if (!host || !v->frames || !wide.get(device, BlockPool::kDevice, std::max<size_t>(total, 64)) ||
            !host->get(device, BlockPool::kPinned, std::max<size_t>(total, 64)))
            rc = CCD_ERR_NOMEM;
        if (rc >= 0 && hipEventCreateWithFlags(&frame_done, hipEventDisableTiming) != hipSuccess) rc = CCD_ERR_HIP;
    }
    // planes of display index di: widened to u16 and copied to the host on the copy stream, behind everything enqueued so far
    auto send_frame = [&](int di) -> int {
        const DevFrame& d = dev[di];
        HIP_TRY(hipEventRecord(frame_done, nullptr));
        HIP_TRY(hipStreamWaitEvent(copy_st, frame_done, 0));
        for (int p = 0; p < 3; ++p) {
            const size_t px = p == 0 ? static_cast<size_t>(d.h) * d.w : static_cast<size_t>(d.ch) * d.cw;
            uint16_t* dst = reinterpret_cast<uint16_t*>(wide.as<char>() + off[static_cast<size_t>(di) * 3 + p]);
            const hipError_t e = d.bitdepth == 8 ? launch_widen_u8(static_cast<const uint8_t*>(d.plane[p]), dst, px, copy_st)
                                                 : hipMemcpyAsync(dst, d.plane[p], px * 2, hipMemcpyDeviceToDevice, copy_st);
            if (e != hipSuccess) return CCD_ERR_HIP;
        }
        const size_t o0 = off[static_cast<size_t>(di) * 3], o1 = di + 1 < n_frames ? off[static_cast<size_t>(di + 1) * 3] : total;
        HIP_TRY(hipMemcpyAsync(host->as<char>() + o0, wide.as<char>() + o0, o1 - o0, hipMemcpyDeviceToHost, copy_st));
        return CCD_OK;
    };
    for (int f = 0; f < n_frames && rc >= 0; ++f) {
        const ccd_frame_header& fh = fhs[f];
        DevFrame& d = dev[fh.display_index];
        const Slot& s0 = *b->slots[first_slot[f]];
        if (fh.frame_type == 0) {
            if (s0.hdr.out_channels < 3) { rc = CCD_ERR_VALUE; break; }
            for (int p = 0; p < 3; ++p) d.plane[p] = s0.d_plane[p];
        } else {
            const Slot& s1 = *b->slots[first_slot[f] + 1];
            const int need_res = fh.frame_type == 1 ? 4 : 5, need_mot = fh.frame_type == 1 ? 2 : 4;
            if (s0.hdr.out_channels < need_res || s1.hdr.out_channels < need_mot || s1.hdr.img_size[0] != d.h || s1.hdr.img_size[1] != d.w) { rc = CCD_ERR_VALUE; break; }
            if (fh.warp_filter_size < 2 || fh.warp_filter_size > 16 || (fh.warp_filter_size & 1)) { rc = CCD_ERR_VALUE; break; }  // warp.py:41-56
            const void* refs[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
            for (int k = 0; k < fh.n_refs && rc >= 0; ++k) {
                const int ri = fh.index_references[k];
                // a reference must be a decoded frame of the same geometry AND sample layout: its planes are read with this
                // frame's layout (a 4:2:0 reference has quarter-size chroma planes)
                if (ri < 0 || ri >= n_frames || !dev[ri].plane[0] || dev[ri].h != d.h || dev[ri].w != d.w || dev[ri].bitdepth != d.bitdepth ||
                    dev[ri].fdt != d.fdt) { rc = CCD_ERR_VALUE; break; }
                for (int p = 0; p < 3; ++p) refs[k][p] = dev[ri].plane[p];
            }
            if (rc < 0) break;
            const size_t sb = d.bitdepth == 8 ? 1 : 2;
            const size_t luma = align256(static_cast<size_t>(d.h) * d.w * sb + 16);
            const size_t chroma = align256(static_cast<size_t>(d.ch) * d.cw * sb + 16);
            if (!d.own.get(device, BlockPool::kDevice, luma + 2 * chroma)) { rc = CCD_ERR_NOMEM; break; }
            d.plane[0] = d.own.as<char>(); d.plane[1] = d.own.as<char>() + luma; d.plane[2] = d.own.as<char>() + luma + chroma;
            const size_t need = static_cast<size_t>(9) * d.h * d.w;
            if (need > tmp_elems) {
                if (tmp.p && hipStreamSynchronize(nullptr) != hipSuccess) { rc = CCD_ERR_HIP; break; }  // frames in flight still use the smaller one
                if (!tmp.get(device, BlockPool::kDevice, need * sizeof(float))) { rc = CCD_ERR_NOMEM; break; }
                tmp_elems = need;
            }
            if (coef_done[f] && hipStreamWaitEvent(nullptr, coef_done[f], 0) != hipSuccess) { rc = CCD_ERR_HIP; break; }
            rc = inter_reconstruct_on(nullptr, tmp.as<float>(), fh.frame_type, d.h, d.w, d.bitdepth, d.fdt, s0.d_out, s1.d_out, refs[0],
                                      fh.frame_type == 2 ? refs[1] : nullptr, fh.global_flow, fh.warp_filter_size, d.plane,
                                      coef_done[f] ? coef[f].p : nullptr);
        }
        if (rc >= 0) rc = send_frame(fh.display_index);
    }
    if (timing) { (void)hipStreamSynchronize(nullptr); mark("reconstructed"); }
    if (rc >= 0 && hipStreamSynchronize(copy_st) != hipSuccess) rc = CCD_ERR_HIP;
    mark("planes on the host");
    if (rc >= 0) {
        v->n_frames = n_frames;
        v->frames[n_frames].plane[0] = reinterpret_cast<uint16_t*>(host);  // hidden: the block every plane points into (ccd_video_free)
        for (int f = 0; f < n_frames; ++f) {
            const int di = fhs[f].display_index;
            const DevFrame& d = dev[di];
            ccd_frame& fr = v->frames[di];
            fr.display_index = di; fr.frame_type = fhs[f].frame_type; fr.frame_data_type = d.fdt; fr.bitdepth = d.bitdepth;
            fr.h = d.h; fr.w = d.w; fr.ch = d.ch; fr.cw = d.cw;
            for (int p = 0; p < 3; ++p) fr.plane[p] = reinterpret_cast<uint16_t*>(host->as<char>() + off[static_cast<size_t>(di) * 3 + p]);
        }
    } else {
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
    return rc < 0 ? rc : CCD_OK;
}

}  // extern "C"
