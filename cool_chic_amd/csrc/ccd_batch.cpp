// ccd_batch.cpp - a decode batch behind include/ccd.h: create / destroy, the launches of its three stages, wait, results.
#include <cstdlib>
#include <cstring>
#include <new>

#include "ccd_host.hpp"
#include "ccd_kernels.hpp"

using namespace ccd;

int ccd_batch::drain() {
    int rc = streams.drain();
    // the device's SHARED side streams are not drained (another batch in flight may be launching on them: draining would
    // make this batch's destroy wait for that batch's entropy chains) - this batch's own work on them ends at its events
    for (int k = 0; k < DeviceShared::kSide; ++k)
        if (side_pending[k] && side_done[k]) { if (hipEventSynchronize(side_done[k]) != hipSuccess) rc = CCD_ERR_HIP; side_pending[k] = false; }
    return rc;
}

extern "C" {

int ccd_batch_create(int device, ccd_batch** out) {
    if (!out) return CCD_ERR_ARG;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return CCD_ERR_HIP;
    HIP_TRY(hipSetDevice(device));
    DeviceShared* sh = nullptr;
    const int rc = device_shared(device, &sh);
    if (rc < 0) return rc;
    ccd_batch* b = new (std::nothrow) ccd_batch();
    if (!b) return CCD_ERR_NOMEM;
    b->device = device;
    if (const char* e = std::getenv("CCD_FORCE_GENERIC")) b->force_generic = std::atoi(e);
    if (const char* e = std::getenv("CCD_FUSED_DEC")) {  // 0 / 1 / 2 like the option; anything else leaves the default
        const int v = std::atoi(e);
        if (v >= 0 && v <= 2) b->opt_fused_dec = v;
    }
    if (const char* e = std::getenv("CCD_MFMA_ARM")) b->opt_mfma_arm = std::atoi(e);
    if (const char* e = std::getenv("CCD_FIXED_SHAPE")) b->opt_fixed_shape = std::atoi(e);
    if (const char* e = std::getenv("CCD_OVERLAP")) b->opt_overlap = std::atoi(e);
    b->d_scale_table = sh->d_scale_table;
    b->d_rcp_table = sh->d_rcp_table;
    b->up_stream = sh->up_stream;
    if (hipEventCreateWithFlags(&b->up_done, hipEventDisableTiming) != hipSuccess) { delete b; return CCD_ERR_HIP; }
    *out = b;
    return CCD_OK;
}

void ccd_batch_destroy(ccd_batch* b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    // blocks go back to the pool for the next batch: nothing of this one may still be in flight
    if (b->up_done) { (void)hipEventSynchronize(b->up_done); (void)hipEventDestroy(b->up_done); }
    (void)b->drain();  // launches and copies on EVERY stream the caller used with this batch
    if (b->fork) (void)hipEventDestroy(b->fork);
    if (b->params_up) (void)hipEventDestroy(b->params_up);
    for (hipEvent_t e : b->lg_done) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : b->lt0) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : b->lt1) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : b->side_done) if (e) (void)hipEventDestroy(e);
    for (auto& s : b->slots) { s->arena.release(); s->staging.drop(); }
    b->tables.drop(); b->tables_staging.drop(); b->status_host.drop();
    delete b;
}

int ccd_batch_size(const ccd_batch* b) { return b ? static_cast<int>(b->slots.size()) : CCD_ERR_ARG; }

int ccd_batch_header(const ccd_batch* b, int slot, ccd_cc_header* h) {
    if (!b || !h || slot < 0 || slot >= static_cast<int>(b->slots.size())) return CCD_ERR_ARG;
    *h = b->slots[slot]->hdr;
    return CCD_OK;
}

// Common-randomness planes (coolchic.py:179-183): Gaussian grids at every latent level, then
// fixed_upsampling(mode="bicubic") coarsest -> finest into channels [n_levels, 2 n_levels) of the dense stack.
static int run_common_randomness(Slot& s, hipStream_t st) {
    const int n = static_cast<int>(s.lvl_h.size());
    HIP_TRY(launch_cr_noise(s.d_noise, s.noise_off[n], st));
    const size_t plane0 = static_cast<size_t>(s.dense_h) * s.dense_w;
    // stack at level lv: [target noise lv, upsampled planes of levels lv+1 .. n-1]
    auto stack_at = [&](int lv) { return lv == 0 ? s.d_dense + static_cast<size_t>(n) * plane0 : s.d_nstack[(lv - 1) & 1]; };
    const float* cur = s.d_noise + s.noise_off[n - 1];
    int ch = s.lvl_h[n - 1], cw = s.lvl_w[n - 1], cc = 1;
    if (n == 1) {
        HIP_TRY(hipMemcpyAsync(stack_at(0), cur, plane0 * 4, hipMemcpyDeviceToDevice, st));
        return CCD_OK;
    }
    for (int lv = n - 2; lv >= 0; --lv) {
        const int th = s.lvl_h[lv], tw = s.lvl_w[lv];
        const size_t tp = static_cast<size_t>(th) * tw;
        float* dst = stack_at(lv);  // levels >= 3 fit in the alternating level-1 / level-2 stacks (sizes shrink with lv)
        HIP_TRY(hipMemcpyAsync(dst, s.d_noise + s.noise_off[lv], tp * 4, hipMemcpyDeviceToDevice, st));
        if (th != ch || tw != cw) HIP_TRY(launch_resize_interp(cur, dst + tp, cc, ch, cw, th, tw, 1, 0.5f, 0.5f, st));
        else HIP_TRY(hipMemcpyAsync(dst + tp, cur, static_cast<size_t>(cc) * tp * 4, hipMemcpyDeviceToDevice, st));
        cur = dst; ch = th; cw = tw; ++cc;
    }
    return CCD_OK;
}

static int run_upsampling(Slot& s, hipStream_t st) {
    if (s.cr) { const int rc = run_common_randomness(s, st); if (rc < 0) return rc; }
    if (s.use_fused_dec) return CCD_OK;  // the pyramid is evaluated inside the fused kernel (stage 2)
    if (s.levels.empty()) {
        const int g = [&] { for (int i = 0; i < s.hdr.n_grids; ++i) if (!s.hdr.is_hyperlatent[i]) return i; return 0; }();
        HIP_TRY(launch_i8_to_f32(s.ep.latent[g], s.d_dense, static_cast<size_t>(s.dense_h) * s.dense_w, st));
        return CCD_OK;
    }
    return CCD_OK;  // the pyramid steps were launched for the whole batch (ccd_batch_run_stage)
}

// a slot whose whole float path - fused kernel, final resize, integer planes - can follow its entropy launch on that launch's stream
static bool tail_keyed(const Slot& s) { return s.fl >= 0 && s.use_fused_dec && !s.cr; }

static int run_synthesis(Slot& s, hipStream_t st, bool keyed_done = false) {
    const Network& net = s.net;
    const int h = s.dense_h, w = s.dense_w;
    if (s.use_fused_syn || s.use_fused_dec) {  // the fused kernel itself was launched for the whole group (ccd_batch_run_stage)
        if (keyed_done && tail_keyed(s)) return CCD_OK;  // ... and so were its resize / planes launches (launch_entropy_groups)
        const int H = s.hdr.img_size[0], W = s.hdr.img_size[1];
        if (s.d_out != s.d_syn_out) HIP_TRY(launch_final_resize(s.d_syn_out, s.d_out, s.hdr.out_channels, h, w, H, W, s.hdr.final_upsampling_type, st));
        if (s.bitdepth && !(s.use_fused_dec ? s.fdec.write_planes : s.fused.write_planes))
            HIP_TRY(launch_planes(s.d_out, s.d_plane[0], s.d_plane[1], s.d_plane[2], H, W, s.bitdepth, s.frame_data_type, st));
        return CCD_OK;
    }
    const float* x = s.d_dense;
    int cur = 0;
    for (size_t l = 0; l < net.syn.size(); ++l) {
        const SynLayerParams& L = net.syn[l];
        HIP_TRY(launch_syn_layer(x, nullptr, s.d_syn_params + s.w_off[l], s.d_syn_params + s.b_off[l], s.d_tmp[cur], L.c_in,
                                 L.c_out, L.k, L.residual, L.relu, h, w, st));
        x = s.d_tmp[cur];
        cur ^= 1;
    }
    const float* stab = nullptr;
    if (net.syn_stab.c_out) {
        HIP_TRY(launch_syn_layer(s.d_dense, nullptr, s.d_syn_params + s.stab_w, s.d_syn_params + s.stab_b, s.d_stab,
                                 net.syn_stab.c_in, net.syn_stab.c_out, 1, 0, 0, h, w, st));
        stab = s.d_stab;
    }
    HIP_TRY(launch_syn_layer(x, stab, s.d_syn_params + s.out_w, s.d_syn_params + s.out_b, s.d_syn_out, net.syn_out.c_in,
                             net.syn_out.c_out, 1, 0, 0, h, w, st));
    const int H = s.hdr.img_size[0], W = s.hdr.img_size[1];
    if (s.d_out != s.d_syn_out)
        HIP_TRY(launch_final_resize(s.d_syn_out, s.d_out, s.hdr.out_channels, h, w, H, W, s.hdr.final_upsampling_type, st));
    if (s.bitdepth)
        HIP_TRY(launch_planes(s.d_out, s.d_plane[0], s.d_plane[1], s.d_plane[2], H, W, s.bitdepth, s.frame_data_type, st));
    return CCD_OK;
}

// Entropy launches of a batch (and, with `with_float`, each launch's own float-path launches right behind it) forked over the
// device's side streams and joined on `st`.  Launch 0 - the one with the longest expected chains - stays on the caller's stream.
// With ONE launch there is nothing to fork: it goes to `st` and the float stages follow it there (the caller enqueues them).
static int launch_entropy_groups(ccd_batch* b, hipStream_t st, bool with_float) {
    // launch order: longest expected chains first (they start first where launches queue behind each other)
    std::vector<int> order(b->pipe_groups.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = static_cast<int>(i);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return b->pipe_groups[x].est > b->pipe_groups[y].est; });
    const int n_launch = static_cast<int>(order.size()) + (b->n_generic > 0 ? 1 : 0);
    DeviceShared* sh = nullptr;
    if (n_launch > 1) {
        const int rc = device_shared(b->device, &sh);
        if (rc < 0) return rc;
        if (!b->fork) HIP_TRY(hipEventCreateWithFlags(&b->fork, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(b->fork, st));
    }
    std::vector<int> used;
    // one launch: the caller's stream.  Several: ALL of them on the side streams that were measured to run concurrently
    // (DeviceShared::conc), launch k on conc[k mod n_conc] - the caller's stream only forks and joins.
    auto stream_for = [&](int idx, int* side_out) -> hipStream_t {
        *side_out = -1;
        if (!sh) return st;
        const int side = sh->conc[idx % sh->n_conc];
        if (std::find(used.begin(), used.end(), side) == used.end()) {
            used.push_back(side);
            (void)hipStreamWaitEvent(sh->side[side], b->fork, 0);
        }
        *side_out = side;
        return sh->side[side];
    };
    // an event behind everything this batch has put on a side stream so far: what a destroy / a table replacement waits for, also
    // after an error between the fork and the join below (the shared side streams themselves are never drained)
    auto mark = [&](int side) -> int {
        if (side < 0) return CCD_OK;
        if (!b->side_done[side]) HIP_TRY(hipEventCreateWithFlags(&b->side_done[side], hipEventDisableTiming));
        HIP_TRY(hipEventRecord(b->side_done[side], sh->side[side]));
        b->side_pending[side] = true;
        return CCD_OK;
    };
    int k = 0;
    if (b->opt_time_launches) {
        while (static_cast<int>(b->lt0.size()) < n_launch) {
            hipEvent_t e0 = nullptr, e1 = nullptr;
            HIP_TRY(hipEventCreate(&e0));
            b->lt0.push_back(e0);
            HIP_TRY(hipEventCreate(&e1));
            b->lt1.push_back(e1);
        }
        b->n_timed = n_launch;
    }
    for (int gi : order) {
        const auto& g = b->pipe_groups[gi];
        int side = -1;
        const int kk = k;
        hipStream_t s = stream_for(k++, &side);
        if (b->opt_time_launches) HIP_TRY(hipEventRecord(b->lt0[kk], s));
        hipError_t e = launch_entropy_pipe(b->d_params + g.first, g.n, g.nv, g.mfma, g.dyn, g.shape, g.lds, s);
        if (b->opt_time_launches) HIP_TRY(hipEventRecord(b->lt1[kk], s));
        if (e == hipSuccess && with_float) {
            // this launch's frames: pyramid launch(es), then the fused kernel - on the SAME stream, so they start when this launch's
            // slowest stream is done, whatever the other launches are doing.  (Common randomness needs its noise planes first:
            // those groups run behind the join like every per-slot launch.)
            for (const auto& pg : b->pyr_groups)
                if (pg.fl == gi && e == hipSuccess)
                    e = launch_fused_pyramid(b->d_pyr + pg.first_frame, static_cast<const char*>(b->d_pyr_work) + static_cast<size_t>(pg.first_work) * 16, pg.n_work, pg.levels, pg.lds, s);
            for (const auto& fg : b->fdec_groups)
                if (fg.fl == gi && !fg.cr && e == hipSuccess)
                    e = launch_fused_dec(b->d_fdec + fg.first_frame, static_cast<const char*>(b->d_fdec_work) + static_cast<size_t>(fg.first_work) * 16, fg.n_work, fg.c_in, fg.c, fg.pre, fg.lds, s);
        }
        if (e == hipSuccess && with_float) {
            // ... and what follows the fused kernel per slot: the final resize (the motion cool-chics' nearest x 4) and, where the
            // fused kernel did not write them, the integer planes
            for (auto& sp : b->slots)
                if (sp->lg == gi && tail_keyed(*sp) && run_synthesis(*sp, s) < 0) { e = hipErrorUnknown; break; }
        }
        if (e == hipSuccess && with_float) {
            while (b->lg_done.size() <= static_cast<size_t>(gi)) b->lg_done.push_back(nullptr);
            if (!b->lg_done[gi] && hipEventCreateWithFlags(&b->lg_done[gi], hipEventDisableTiming) != hipSuccess) e = hipErrorUnknown;
            if (e == hipSuccess) e = hipEventRecord(b->lg_done[gi], s);
        }
        const int rc = mark(side);
        if (e != hipSuccess) return CCD_ERR_HIP;
        if (rc < 0) return rc;
    }
    b->lg_valid = with_float;
    if (b->n_generic > 0) {
        int side = -1;
        const int kk = k;
        hipStream_t s = stream_for(k++, &side);
        if (b->opt_time_launches) HIP_TRY(hipEventRecord(b->lt0[kk], s));
        const hipError_t e = launch_entropy(b->d_params + b->n_pipe, b->n_generic, b->lds_generic, s);
        if (b->opt_time_launches) HIP_TRY(hipEventRecord(b->lt1[kk], s));
        const int rc = mark(side);
        if (e != hipSuccess) return CCD_ERR_HIP;
        if (rc < 0) return rc;
    }
    for (int side : used) HIP_TRY(hipStreamWaitEvent(st, b->side_done[side], 0));
    return CCD_OK;
}

// the float-path launches of stage 1 / stage 2 that belong to the whole batch; `keyed_done`: the pyramid / fused launches keyed by
// an entropy launch were already enqueued behind it (launch_entropy_groups with_float)
static int launch_float_stage(ccd_batch* b, hipStream_t st, int stage, bool keyed_done) {
    if (stage == 1) {
        for (const auto& u : b->ups_steps)
            HIP_TRY(launch_upsample_step(b->d_levels, b->d_zmap + u.first_z, u.n_z, u.max_w, u.max_h, st));
        for (const auto& g : b->pyr_groups) {
            if (keyed_done && g.fl >= 0) continue;
            HIP_TRY(launch_fused_pyramid(b->d_pyr + g.first_frame, static_cast<const char*>(b->d_pyr_work) + static_cast<size_t>(g.first_work) * 16,
                                         g.n_work, g.levels, g.lds, st));
        }
    }
    if (stage == 2) {
        for (const auto& g : b->fused_groups)
            HIP_TRY(launch_syn_fused(b->d_fused + g.first, g.n, g.c_in, g.c, g.max_tx, g.max_ty, st));
        for (const auto& g : b->fdec_groups) {
            if (keyed_done && g.fl >= 0 && !g.cr) continue;
            const FusedDec* fr = b->d_fdec + g.first_frame;
            const char* wk = static_cast<const char*>(b->d_fdec_work) + static_cast<size_t>(g.first_work) * 16;
            if (g.cr) HIP_TRY(launch_fused_dec_cr(fr, wk, g.n_work, g.c_in, g.c, g.lds, st));
            else HIP_TRY(launch_fused_dec(fr, wk, g.n_work, g.c_in, g.c, g.pre, g.lds, st));
        }
    }
    for (auto& sp : b->slots) {
        const int rc = (stage == 1) ? run_upsampling(*sp, st) : run_synthesis(*sp, st, keyed_done);
        if (rc < 0) return rc;
    }
    return CCD_OK;
}

// common head of a run: device, the slots' uploads, the launch tables (and their copy, if another stream carried it)
static int run_prologue(ccd_batch* b, hipStream_t st) {
    HIP_TRY(hipSetDevice(b->device));
    if (b->uploads_unconfirmed) HIP_TRY(hipStreamWaitEvent(st, b->up_done, 0));  // the slots' uploads (ccd_batch_add) come first
    b->streams.note(st);
    const int rc = build_launch_tables(b, st);
    if (rc < 0) return rc;
    if (b->params_up && b->params_stream != st) HIP_TRY(hipStreamWaitEvent(st, b->params_up, 0));
    b->run_stream = st;
    b->has_run = true;
    return CCD_OK;
}

// head of stage 0: the grids of the slots whose latents are device pointers are read NOW, into the slots' arenas - one launch
static int launch_ingest(ccd_batch* b, hipStream_t st) {
    if (!b->n_ingest) return CCD_OK;
    const int word = (b->ingest_runs & 1) ? kIngestWordB : 0;
    HIP_TRY(launch_latent_ingest(b->d_ingest, b->d_ingest_prefix, b->n_ingest, b->n_ingest_blocks, b->d_status_all, word, st));
    ++b->ingest_runs;
    return CCD_OK;
}

int ccd_batch_run_stage(ccd_batch* b, void* stream, int stage) {
    if (!b || stage < 0 || stage > 2) return CCD_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = run_prologue(b, st);
    if (rc < 0) return rc;
    // stage 0: one launch per kernel instantiation and chain group in use.  The first goes to the caller's stream; the others fork
    // to side streams and join again, so that they overlap (each stream of a launch occupies one CU for its whole serial chain:
    // queued on one stream, a GOP whose I frames need another instantiation than its B frames took the SUM of the two).
    if (stage == 0) {
        const int ri = launch_ingest(b, st);
        return ri < 0 ? ri : launch_entropy_groups(b, st, false);
    }
    return launch_float_stage(b, st, stage, false);
}

int ccd_batch_prepare(ccd_batch* b, void* stream) {
    if (!b) return CCD_ERR_ARG;
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    b->streams.note(st);
    return build_launch_tables(b, st);
}

// All three stages.  Unlike three ccd_batch_run_stage calls, the float path of a frame does not wait for the slowest stream of
// the BATCH: every entropy launch (kernel instantiation x chain group, build_launch_tables) is followed on its own stream by the
// pyramid + fused launches of its own frames, and the streams join once at the end (decode.py:67-81: frames are independent).
int ccd_batch_run(ccd_batch* b, void* stream) {
    if (!b) return CCD_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = run_prologue(b, st);
    if (rc < 0) return rc;
    const bool overlap = b->opt_overlap && b->pipe_groups.size() + (b->n_generic > 0 ? 1 : 0) > 1;
    rc = launch_ingest(b, st);  // given slots: their float launches are keyed to no entropy launch and follow on `st`
    if (rc < 0) return rc;
    rc = launch_entropy_groups(b, st, overlap);
    if (rc < 0) return rc;
    for (int stage = 1; stage <= 2; ++stage) {
        rc = launch_float_stage(b, st, stage, overlap);
        if (rc < 0) return rc;
    }
    return CCD_OK;
}

int ccd_batch_wait(ccd_batch* b, void* stream) {
    if (!b) return CCD_ERR_ARG;
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    b->streams.note(st);
    // the status words and the results are behind the run on the stream the run was given, whichever stream this call names
    if (b->has_run && b->run_stream != st) HIP_TRY(hipStreamSynchronize(b->run_stream));
    // slots added after the last run have no status yet: the words of the slots that DID run are refreshed all the same (their
    // array and its pinned copy were sized for them)
    const size_t n = std::min(b->slots.size(), static_cast<size_t>(b->n_params_uploaded));
    if (n && b->d_status_all) {
        // the status words of all slots are one array: one copy into pinned memory, one wait
        HIP_TRY(hipMemcpyAsync(b->status_host.p, b->d_status_all, n * 64 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (n == b->slots.size()) b->uploads_unconfirmed = false;  // every launch behind the uploads has finished
        const int32_t* hs = b->status_host.as<int32_t>();
        int first = CCD_OK;
        for (size_t i = 0; i < n; ++i) {
            Slot& sl = *b->slots[i];
            std::memcpy(sl.host_status, hs + i * 64, sizeof(sl.host_status));
            if (sl.given_device && b->ingest_runs) {  // the word the LAST ingest launch reported into (ccd_ingest.hip)
                sl.host_status[0] = sl.host_status[((b->ingest_runs - 1) & 1) ? kIngestWordB : 0];
                sl.host_status[kIngestWordB] = 0;
            }
            sl.status = sl.host_status[0];
            if (first == CCD_OK && sl.status != CCD_OK) first = sl.status;
        }
        return first;
    }
    HIP_TRY(hipStreamSynchronize(st));  // nothing was run yet
    return CCD_OK;
}

int ccd_batch_slot_status(const ccd_batch* b, int slot) {
    if (!b || slot < 0 || slot >= static_cast<int>(b->slots.size())) return CCD_ERR_ARG;
    return b->slots[slot]->status;
}

int ccd_batch_slot_stats(const ccd_batch* b, int slot, int32_t* out64) {
    if (!b || !out64 || slot < 0 || slot >= static_cast<int>(b->slots.size())) return CCD_ERR_ARG;
    std::memcpy(out64, b->slots[slot]->host_status, sizeof(b->slots[slot]->host_status));
    return CCD_OK;
}

int ccd_batch_launch_ms(ccd_batch* b, float* ms, int* n_streams, int cap) {
    if (!b || !ms || cap < 0) return CCD_ERR_ARG;
    if (!b->opt_time_launches) return 0;
    // launch order = longest expected chains first (launch_entropy_groups); the generic launch last
    std::vector<int> order(b->pipe_groups.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = static_cast<int>(i);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return b->pipe_groups[x].est > b->pipe_groups[y].est; });
    const int n = std::min(b->n_timed, cap);
    for (int k = 0; k < n; ++k) {
        if (hipEventSynchronize(b->lt1[k]) != hipSuccess || hipEventElapsedTime(&ms[k], b->lt0[k], b->lt1[k]) != hipSuccess) return CCD_ERR_HIP;
        if (n_streams) n_streams[k] = k < static_cast<int>(order.size()) ? b->pipe_groups[order[k]].n : b->n_generic;
    }
    return n;
}

int ccd_batch_entropy_launches(const ccd_batch* b) {
    if (!b) return CCD_ERR_ARG;
    return static_cast<int>(b->pipe_groups.size()) + (b->n_generic > 0 ? 1 : 0);
}

int ccd_batch_slot_kernels(const ccd_batch* b, int slot) {
    if (!b || slot < 0 || slot >= static_cast<int>(b->slots.size())) return CCD_ERR_ARG;
    const Slot& s = *b->slots[slot];
    return (s.use_pipe ? 1 : 0) | (s.use_fused_syn ? 2 : 0) | (s.use_fused_dec ? 4 : 0) | (s.use_mfma ? 8 : 0) | (s.use_dyn ? 16 : 0) | (s.fixed_shape ? 32 : 0) | (s.fdec_pre ? 64 : 0) | (s.float_finite ? 0 : 128) | (s.given ? 256 : 0);
}

const float* ccd_batch_output(const ccd_batch* b, int slot) {
    if (!b || slot < 0 || slot >= static_cast<int>(b->slots.size())) return nullptr;
    const Slot& s = *b->slots[slot];
    if (s.use_fused_dec && !s.fdec.out) return nullptr;  // CCD_OPT_KEEP_FLOAT = 0: integer samples only
    return s.d_out;
}
const float* ccd_batch_dense(const ccd_batch* b, int slot) {
    // the dense stack only exists on the unfused path (ccd_batch_set_option(b, CCD_OPT_FUSED_DEC, 0) before adding the slot)
    return (b && slot >= 0 && slot < static_cast<int>(b->slots.size()) && !b->slots[slot]->use_fused_dec) ? b->slots[slot]->d_dense : nullptr;
}
int ccd_batch_set_option(ccd_batch* b, int option, int value) {
    if (!b) return CCD_ERR_ARG;
    switch (option) {
        case CCD_OPT_FUSED_DEC:
            if (value < 0 || value > 2) return CCD_ERR_ARG;
            b->opt_fused_dec = value; return CCD_OK;
        case CCD_OPT_KEEP_FLOAT: b->opt_keep_float = value; return CCD_OK;
        case CCD_OPT_MFMA_ARM: b->opt_mfma_arm = value; return CCD_OK;
        case CCD_OPT_RANGE_BITS: b->opt_range_bits = value; return CCD_OK;
        case CCD_OPT_TIME_LAUNCHES: b->opt_time_launches = value ? 1 : 0; return CCD_OK;
        case CCD_OPT_OVERLAP:
            // (decides how the launch tables are grouped: a change re-builds them at the next run)
            if (b->opt_overlap != (value ? 1 : 0)) { b->opt_overlap = value ? 1 : 0; b->regroup = true; }
            return CCD_OK;
        default: return CCD_ERR_ARG;
    }
}
const int8_t* ccd_batch_latent(const ccd_batch* b, int slot, int grid) {
    if (!b || slot < 0 || slot >= static_cast<int>(b->slots.size())) return nullptr;
    const Slot& s = *b->slots[slot];
    return (grid >= 0 && grid < s.hdr.n_grids) ? s.ep.latent[grid] : nullptr;
}
const void* ccd_batch_plane(const ccd_batch* b, int slot, int plane, int* h, int* w) {
    if (!b || slot < 0 || slot >= static_cast<int>(b->slots.size()) || plane < 0 || plane > 2) return nullptr;
    const Slot& s = *b->slots[slot];
    if (h) *h = s.plane_h[plane];
    if (w) *w = s.plane_w[plane];
    return s.d_plane[plane];
}

// Results of a slot whose entropy stage reported an error (corrupt / truncated payload) are whatever the arena held: never
// handed out.  (Status is known after ccd_batch_wait; before it the copy reflects the caller's own ordering.)
static int slot_failed(const ccd_batch* b, int slot) {
    return (b && slot >= 0 && slot < static_cast<int>(b->slots.size()) && b->slots[slot]->status < 0) ? b->slots[slot]->status : 0;
}

static int copy_out(ccd_batch* b, const void* src, void* dst, size_t bytes, void* stream) {
    if (!src || !dst) return CCD_ERR_ARG;
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    b->streams.note(st);
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return CCD_OK;
}

int ccd_batch_copy_latent(ccd_batch* b, int slot, int grid, int8_t* host, void* stream) {
    if (const int failed = slot_failed(b, slot)) return failed;
    const int8_t* p = ccd_batch_latent(b, slot, grid);
    if (!p) return CCD_ERR_ARG;
    const ccd_cc_header& h = b->slots[slot]->hdr;
    return copy_out(b, p, host, static_cast<size_t>(h.grid_h[grid]) * h.grid_w[grid], stream);
}
int ccd_batch_copy_plane(ccd_batch* b, int slot, int plane, void* host, void* stream) {
    if (const int failed = slot_failed(b, slot)) return failed;
    int ph = 0, pw = 0;
    const void* p = ccd_batch_plane(b, slot, plane, &ph, &pw);
    if (!p) return CCD_ERR_ARG;
    return copy_out(b, p, host, static_cast<size_t>(ph) * pw * (b->slots[slot]->bitdepth == 8 ? 1 : 2), stream);
}
int ccd_batch_planes_layout(const ccd_batch* b, int slot, size_t* total_bytes, size_t* off3) {
    if (!b || slot < 0 || slot >= static_cast<int>(b->slots.size())) return CCD_ERR_ARG;
    const Slot& s = *b->slots[slot];
    if (!s.d_plane[0]) return CCD_ERR_ARG;  // added with bitdepth = 0
    if (total_bytes) *total_bytes = s.planes_bytes;
    if (off3) for (int p = 0; p < 3; ++p) off3[p] = s.plane_off[p];
    return CCD_OK;
}

int ccd_batch_copy_planes_async(ccd_batch* b, int first_slot, int n_slots, void* const* host_blocks, void* stream) {
    if (!b || !host_blocks || first_slot < 0 || n_slots < 0 || first_slot + n_slots > static_cast<int>(b->slots.size())) return CCD_ERR_ARG;
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    b->streams.note(st);  // the copies read the arenas: drained before the blocks are recycled (ccd_batch_destroy)
    int rc = CCD_OK;
    for (int i = 0; i < n_slots; ++i) {
        const Slot& s = *b->slots[first_slot + i];
        if (!s.d_plane[0] || !host_blocks[i]) { if (rc == CCD_OK) rc = CCD_ERR_ARG; continue; }
        if (s.status < 0) { if (rc == CCD_OK) rc = s.status; continue; }  // a failed slot's planes are never handed out
        if (hipMemcpyAsync(host_blocks[i], s.d_plane[0], s.planes_bytes, hipMemcpyDeviceToHost, st) != hipSuccess) return CCD_ERR_HIP;
    }
    return rc;
}

int ccd_batch_copy_output(ccd_batch* b, int slot, float* host, void* stream) {
    if (const int failed = slot_failed(b, slot)) return failed;
    const float* p = ccd_batch_output(b, slot);
    if (!p) return CCD_ERR_ARG;
    const ccd_cc_header& h = b->slots[slot]->hdr;
    return copy_out(b, p, host, static_cast<size_t>(h.out_channels) * h.img_size[0] * h.img_size[1] * 4, stream);
}
int ccd_batch_copy_dense(ccd_batch* b, int slot, float* host, void* stream) {
    if (const int failed = slot_failed(b, slot)) return failed;
    const float* p = ccd_batch_dense(b, slot);
    if (!p) return CCD_ERR_ARG;
    const Slot& s = *b->slots[slot];
    return copy_out(b, p, host, static_cast<size_t>(s.dense_c) * s.dense_h * s.dense_w * 4, stream);
}
}  // extern "C"
