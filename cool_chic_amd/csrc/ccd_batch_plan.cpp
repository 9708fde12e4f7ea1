// ccd_batch_plan.cpp - from bytes to descriptors and launch tables: ccd_batch_add lays a cool-chic out in its arena, and
// build_launch_tables groups the slots of a batch into launches and uploads the tables those launches read.
#include <array>
#include <cstdlib>
#include <cstring>
#include <new>

#include "ccd_host.hpp"
#include "ccd_kernels.hpp"
#include "ccd_wavefront.hpp"

using namespace ccd;

namespace ccd {
void pack_int_networks(const ccd_cc_header& h, const Network& net, IntNetBlobs& out) {
    for (const FixedLayer& L : net.arm.layers) {
        out.arm.insert(out.arm.end(), L.w.begin(), L.w.end());
        out.arm.insert(out.arm.end(), L.b.begin(), L.b.end());
    }
    out.arm.insert(out.arm.end(), net.arm.ws.begin(), net.arm.ws.end());
    out.arm.insert(out.arm.end(), net.arm.bs.begin(), net.arm.bs.end());
    out.ifce_off.assign(h.n_grids, 0);
    for (int g = 0; g < h.n_grids; ++g) {
        if (net.ifce[g].dim == 0) continue;
        out.ifce_off[g] = static_cast<int32_t>(out.ifce.size());
        const FixedLayer& L = net.ifce[g].layers[0];
        out.ifce.insert(out.ifce.end(), L.w.begin(), L.w.end());
        out.ifce.insert(out.ifce.end(), L.b.begin(), L.b.end());
    }
}
// What of EntropyParams follows from the header and the network alone: grid geometry, levels, the ARM's shape, the context
// template.  Pointers and the kernel-specific fields are the caller's.
void fill_entropy_model(const ccd_cc_header& h, const Network& net, const IntNetBlobs& blobs, EntropyParams& E) {
    E.n_grids = h.n_grids;
    int level = 0;
    for (int g = 0; g < h.n_grids; ++g) {
        E.grid_h[g] = h.grid_h[g]; E.grid_w[g] = h.grid_w[g];
        E.ifce_in[g] = h.input_features_ifce[g];
        E.ifce_off[g] = blobs.ifce_off[g];
        if (g > 0 && (h.grid_h[g] != h.grid_h[g - 1] || h.grid_w[g] != h.grid_w[g - 1])) ++level;
        E.level[g] = level;
    }
    E.dim = h.total_context_arm; E.n_spatial = h.spatial_context_arm; E.n_ifce_out = h.output_feature_ifce;
    E.n_layers = h.n_hidden_layers_arm + 1;
    E.narrow = net.arm.narrow ? 1 : 0;
    E.has_ifce = h.has_ifce_resolution;
    context_offsets(h.spatial_context_arm, E.ctx_dy, E.ctx_dx);
    E.arm_len = static_cast<int32_t>(blobs.arm.size());
}
// The header parses, but the reference cannot decode it: after ONE x2 nearest upsample + crop of the decoded stack its
// torch.cat raises when consecutive grids differ by more than one level (latent and hyperlatent ranges that do not
// touch).  The entropy kernels index the coarser grid with (y >> 1, x >> 1): a larger gap would read past it.
bool grids_nest(const ccd_cc_header& h) {
    for (int g = 1; g < h.n_grids; ++g) {
        const bool same = h.grid_h[g] == h.grid_h[g - 1] && h.grid_w[g] == h.grid_w[g - 1];
        const bool half = h.grid_h[g] == (h.grid_h[g - 1] + 1) / 2 && h.grid_w[g] == (h.grid_w[g - 1] + 1) / 2;
        if (!same && !half) return false;
    }
    return true;
}
}  // namespace ccd

namespace {
// Where everything of a slot sits: byte offsets into its arena, in the order they were reserved (layout_arena), and the
// fused float path's parameter block as a float offset into the synthesis parameters.
struct SlotLayout {
    size_t status = 0, words = 0, arm = 0, ifce = 0, synp = 0, head_bytes = 0;
    std::vector<size_t> lat;  // per grid
    size_t feat = 0, feat_elems = 0, noise = 0, nstack[2] = {0, 0};
    size_t stack_a = 0, stack_b = 0, tmp0 = 0, tmp1 = 0, stab = 0, synout = 0, out = 0, planes = 0;
    size_t fdec_params = 0;
};
// What ccd_batch_add works out about a slot on the host before anything is placed on the device.
struct SlotPlan {
    IntNetBlobs blobs;
    size_t n_words = 0;            // of the payload
    std::vector<int> lat_grids;    // the grids that are latents, finest first
    int n_levels = 0, max_c = 0;
    bool need_resize = false;
    std::vector<float> syn_blob;   // synthesis parameters: the layers as transmitted, then the fused kernels' own copies
    const int8_t* const* host_latents = nullptr;  // given latents on the host: they go up with the head
    SlotLayout at;
};

// ---- 1. header and networks ------------------------------------------------------------------------------------------
int parse_slot(Slot& s, const uint8_t* cc_header, size_t n_hdr, const uint8_t* bytes_nn, size_t n_nn, size_t n_lat, int bitdepth, int frame_data_type) {
    int rc = read_cc_header(cc_header, n_hdr, &s.hdr);
    if (rc < 0) return rc;
    if (n_lat % 4) return CCD_ERR_VALUE;  // np.frombuffer(dtype=uint32) raises (rangecoder.py:81)
    // (The transmitted n_latent_grids is not checked: the reference recomputes the count from the resolutions and never
    // reads the field, component/core/coolchic.py:170-185, header.py:354-377.)
    if (!grids_nest(s.hdr)) return CCD_ERR_VALUE;
    rc = decode_network(s.hdr, bytes_nn, n_nn, s.net);
    if (rc < 0) return rc;
    s.bitdepth = bitdepth; s.frame_data_type = frame_data_type;
    return CCD_OK;
}

// ---- 2. pack the integer networks, choose the entropy kernel's instantiation ---------------------------------------------
int choose_entropy_kernel(const ccd_batch* b, Slot& s, SlotPlan& p) {
    const ccd_cc_header& h = s.hdr;
    const Network& net = s.net;
    pack_int_networks(h, net, p.blobs);
    int max_w = 0;
    for (int g = 0; g < h.n_grids; ++g) max_w = std::max(max_w, static_cast<int>(h.grid_w[g]));
    s.use_pipe = !b->force_generic && entropy_pipe_supports(h.total_context_arm, h.n_hidden_layers_arm + 1, (net.arm.w32 && net.feat_i32 && !net.arm.dyn_act) ? 1 : 0, max_w);
    s.use_mfma = s.use_pipe && b->opt_mfma_arm &&
                 entropy_pipe_supports_mfma(h.total_context_arm, h.n_hidden_layers_arm + 1, h.output_feature_ifce, net.arm.narrow ? 1 : 0, max_w,
                                            arm_max_abs_weight(net.arm), worst_feature_bound(net));
    s.use_dyn = s.use_pipe && !s.use_mfma && (net.arm.dyn_feat || b->opt_range_bits != 0);
    s.fixed_shape = (s.use_pipe && !s.use_mfma && b->opt_fixed_shape) ? entropy_pipe_fixed_shape(h.total_context_arm, h.n_hidden_layers_arm + 1, h.spatial_context_arm) : 0;
    s.ring_rows = s.use_mfma ? std::max(entropy_pipe_ring_rows(max_w), 64) : 512;  // the matrix-core variant needs the LDS for its operand tables
    s.lds_pipe = entropy_pipe_lds_bytes(h.total_context_arm, h.n_hidden_layers_arm + 1, s.ring_rows, s.use_mfma ? 1 : 0);
    s.lds_generic = entropy_lds_bytes(h.total_context_arm, static_cast<int>(p.blobs.arm.size()));
    if (!s.use_pipe && s.lds_generic > 160 * 1024) return CCD_ERR_UNSUPPORTED;  // ARM too large for the LDS-resident kernels
    return CCD_OK;
}

// ---- ... geometry of the float stages, and what the reference refuses about it ------------------------------------------
int float_geometry(Slot& s, SlotPlan& p) {
    const ccd_cc_header& h = s.hdr;
    for (int g = 0; g < h.n_grids; ++g) if (!h.is_hyperlatent[g]) p.lat_grids.push_back(g);
    const int n_levels = p.n_levels = static_cast<int>(p.lat_grids.size());
    s.cr = h.flag_common_randomness != 0;
    if (n_levels < 1 || n_levels * (s.cr ? 2 : 1) != h.input_feature_synthesis) return CCD_ERR_VALUE;
    if (n_levels > 1 && s.net.n_ups < 1) return CCD_ERR_VALUE;
    s.dense_c = h.input_feature_synthesis; s.dense_h = h.grid_h[p.lat_grids[0]]; s.dense_w = h.grid_w[p.lat_grids[0]];
    p.need_resize = (s.dense_h != h.img_size[0] || s.dense_w != h.img_size[1]);
    // the reference concatenates [.., dense_h, dense_w] with noise resized to img_size: torch.cat raises unless equal
    if (s.cr && p.need_resize) return CCD_ERR_VALUE;
    if (s.bitdepth != 0 && h.out_channels < 3) return CCD_ERR_ARG;
    return CCD_OK;
}

// ---- 3. synthesis parameters: the layers as transmitted, then the fused-synthesis layout (zero-padded copies of the first
// two layers and the stabiliser) ------------------------------------------------------------------------------------------
void layout_synthesis(const ccd_batch* b, Slot& s, SlotPlan& p) {
    const ccd_cc_header& h = s.hdr;
    const Network& net = s.net;
    std::vector<float>& syn_blob = p.syn_blob;
    auto push = [&](const std::vector<float>& v) { size_t off = syn_blob.size(); syn_blob.insert(syn_blob.end(), v.begin(), v.end()); return off; };
    s.w_off.clear(); s.b_off.clear();
    p.max_c = h.out_channels;
    for (const SynLayerParams& L : net.syn) { s.w_off.push_back(push(L.w)); s.b_off.push_back(push(L.b)); p.max_c = std::max(p.max_c, L.c_out); }
    if (net.syn_stab.c_out) { s.stab_w = push(net.syn_stab.w); s.stab_b = push(net.syn_stab.b); }
    s.out_w = push(net.syn_out.w); s.out_b = push(net.syn_out.b);
    SynthFused& F = s.fused;
    std::memset(&F, 0, sizeof(F));
    const auto& L = net.syn;
    bool ok = L.size() >= 2 && L.size() <= 5 && L[0].k == 1 && L[1].k == 1 && !L[0].residual && !L[1].residual &&
              L[1].c_out == h.out_channels && !b->force_generic;
    int halo = 0;
    for (size_t l = 2; ok && l < L.size(); ++l) {
        ok = L[l].c_in == h.out_channels && L[l].c_out == h.out_channels && (L[l].k & 1) && L[l].k <= 7;
        halo += (L[l].k - 1) / 2;
    }
    ok = ok && syn_fused_supports(s.dense_c, h.out_channels, halo) && (!net.syn_stab.c_out || net.syn_stab.c_in <= s.dense_c);
    if (ok) {
        const int cp = ((s.dense_c + 3) / 4) * 4, C = h.out_channels, N = L[0].c_out;
        auto push_padded = [&](const std::vector<float>& w, int rows, int cols) {
            const size_t off = syn_blob.size();
            for (int r = 0; r < rows; ++r)
                for (int c = 0; c < cp; ++c) syn_blob.push_back(c < cols ? w[static_cast<size_t>(r) * cols + c] : 0.0f);
            return static_cast<int32_t>(off);
        };
        F.c_in = s.dense_c; F.c = C; F.n_hidden = N; F.relu0 = L[0].relu; F.relu1 = L[1].relu;
        F.w0_off = push_padded(L[0].w, N, s.dense_c); F.b0_off = static_cast<int32_t>(s.b_off[0]);
        F.w1_off = static_cast<int32_t>(s.w_off[1]); F.b1_off = static_cast<int32_t>(s.b_off[1]);
        F.n_conv = static_cast<int32_t>(L.size()) - 2;
        for (int l = 0; l < F.n_conv; ++l) {
            F.conv_k[l] = L[l + 2].k; F.conv_residual[l] = L[l + 2].residual; F.conv_relu[l] = L[l + 2].relu;
            F.conv_w_off[l] = static_cast<int32_t>(s.w_off[l + 2]); F.conv_b_off[l] = static_cast<int32_t>(s.b_off[l + 2]);
        }
        F.has_stab = net.syn_stab.c_out ? 1 : 0;
        if (F.has_stab) {
            F.stab_c_in = net.syn_stab.c_in;
            F.stab_w_off = push_padded(net.syn_stab.w, C, net.syn_stab.c_in);
            F.stab_b_off = static_cast<int32_t>(s.stab_b);
        }
        F.out_w_off = static_cast<int32_t>(s.out_w); F.out_b_off = static_cast<int32_t>(s.out_b);
        F.halo = halo;
        s.use_fused_syn = true;
    }
}

// ---- 4. fused float path (ccd_fused.hip): parameters in MFMA order, appended to the blob -----------------------------------
void layout_fused_dec(const ccd_batch* b, Slot& s, SlotPlan& p) {
    const ccd_cc_header& h = s.hdr;
    const Network& net = s.net;
    std::vector<float>& syn_blob = p.syn_blob;
    const int n_levels = p.n_levels;
    FusedDec& D = s.fdec;
    std::memset(&D, 0, sizeof(D));
    const auto& L = net.syn;
    const int C = h.out_channels;
    // common randomness: n_levels noise planes behind the latent channels (the kFdPre instantiations with NZ = CIN; pictures only)
    const int NZ = s.cr ? n_levels : 0;
    // the matrix-core kernel is exact for FINITE values (its zero-weight padding: fma(v, 0, acc) == acc); a network that
    // could overflow float32 for some latents runs the vector-ALU kernels, which evaluate the oracle's taps only
    s.float_finite = float_path_stays_finite(net, n_levels, NZ);
    bool ok = b->opt_fused_dec && !b->force_generic && s.float_finite && n_levels + NZ == s.dense_c && n_levels >= 2 && n_levels <= kFdMaxLevels &&
              fused_dec_supports(n_levels, C) && (!s.cr || (b->opt_fused_dec == 2 && fused_dec_cr_supports(n_levels, C))) &&
              net.ups_k == 8 && net.pre_k == 7 && L.size() >= 2 &&
              L.size() <= 2 + static_cast<size_t>(kFdMaxConv) && L[0].k == 1 && L[1].k == 1 && !L[0].residual && !L[1].residual &&
              L[0].c_in == n_levels + NZ && L[1].c_in == L[0].c_out && L[1].c_out == C && (!net.syn_stab.c_out || net.syn_stab.c_in <= n_levels);
    for (size_t l = 2; ok && l < L.size(); ++l) ok = L[l].k == 3 && L[l].c_in == C && L[l].c_out == C;
    if (ok) {
        const int CIN = n_levels, N = L[0].c_out, CT = (C + 3) / 4, NT = (N + 3) / 4;
        const int CI = CIN + NZ;  // inputs of the first 1x1 layer
        int nwv, nws, nwc, nwo;
        fused_dec_param_shape(CIN, C, &nwv, &nws, &nwc, &nwo);
        nwv = (CI + 4 * CT + 15) / 16;
        while (syn_blob.size() % 4) syn_blob.push_back(0.0f);  // the kernel copies the block with 16-byte loads
        const size_t base = syn_blob.size();
        auto alloc = [&](size_t n) { const size_t off = syn_blob.size() - base; syn_blob.resize(syn_blob.size() + n, 0.0f); return static_cast<int32_t>(off); };
        float* P = nullptr;
        auto quad = [&](int32_t off, int q, int i) -> float& { return P[off + q * 4 + i]; };
        D.n_tiles_hidden = NT;
        D.wq_off = alloc(static_cast<size_t>(NT) * nwv * 64); D.b0_off = alloc(static_cast<size_t>(NT) * 4);
        D.b1_off = alloc(static_cast<size_t>(CT) * 4);
        D.stab_off = alloc(static_cast<size_t>(nws) * 64); D.stabb_off = alloc(static_cast<size_t>(CT) * 4);
        D.n_conv = static_cast<int32_t>(L.size()) - 2;
        for (int l = 0; l < D.n_conv; ++l) { D.conv_off[l] = alloc(static_cast<size_t>(nwc) * 64); D.convb_off[l] = alloc(static_cast<size_t>(CT) * 4); }
        D.out_off = alloc(static_cast<size_t>(nwo) * 64); D.outb_off = alloc(static_cast<size_t>(CT) * 4);
        D.n_params = static_cast<int32_t>(syn_blob.size() - base);
        P = syn_blob.data() + base;
        for (int n = 0; n < NT; ++n) {
            const int32_t wq = D.wq_off + n * nwv * 64;
            for (int i = 0; i < 4; ++i) {
                const int hu = 4 * n + i;  // hidden unit = row i of the tile
                if (hu >= N) continue;
                for (int c = 0; c < CI; ++c) quad(wq, c, i) = L[0].w[static_cast<size_t>(hu) * CI + c];
                P[D.b0_off + 4 * n + i] = L[0].b[hu];
            }
            for (int t = 0; t < CT; ++t)
                for (int r = 0; r < 4; ++r)
                    for (int i = 0; i < 4; ++i) {
                        const int oc = 4 * t + i, hu = 4 * n + r;
                        if (oc < C && hu < N) quad(wq, CI + t * 4 + r, i) = L[1].w[static_cast<size_t>(oc) * N + hu];
                    }
        }
        for (int oc = 0; oc < C; ++oc) P[D.b1_off + oc] = L[1].b[oc];
        D.has_stab = net.syn_stab.c_out ? 1 : 0;
        if (D.has_stab)
            for (int oc = 0; oc < C; ++oc) {
                for (int c = 0; c < net.syn_stab.c_in; ++c) quad(D.stab_off, c * CT + oc / 4, oc % 4) = net.syn_stab.w[static_cast<size_t>(oc) * net.syn_stab.c_in + c];
                P[D.stabb_off + oc] = net.syn_stab.b[oc];
            }
        for (int l = 0; l < D.n_conv; ++l) {
            const SynLayerParams& Lc = L[l + 2];
            D.conv_residual[l] = Lc.residual; D.conv_relu[l] = Lc.relu;
            for (int oc = 0; oc < C; ++oc) {
                for (int k = 0; k < 9 * C; ++k) quad(D.conv_off[l], k * CT + oc / 4, oc % 4) = Lc.w[static_cast<size_t>(oc) * 9 * C + k];
                P[D.convb_off[l] + oc] = Lc.b[oc];
            }
        }
        for (int oc = 0; oc < C; ++oc) {
            for (int i = 0; i < C; ++i) quad(D.out_off, i * CT + oc / 4, oc % 4) = net.syn_out.w[static_cast<size_t>(oc) * C + i];
            P[D.outb_off + oc] = net.syn_out.b[oc];
        }
        D.relu0 = L[0].relu; D.relu1 = L[1].relu;
        D.n_lv = n_levels; D.c = C; D.h = s.dense_h; D.w = s.dense_w;
        D.margin = D.n_conv == 0 ? 0 : (D.n_conv <= 2 ? 2 : 4);
        D.tiles_x = (D.w + (64 - 2 * D.margin) - 1) / (64 - 2 * D.margin);
        D.tiles_y = (D.h + (32 - 2 * D.margin) - 1) / (32 - 2 * D.margin);
        // kron products of the symmetric 1-D filters (upsampling.py:42-64, 189-196, 312-325): level i is produced by step
        // n_levels - 2 - i (coarsest first), whose filters are those of index step % n_ups
        for (int i = 0; i + 1 < n_levels; ++i) {
            const int kidx = (n_levels - 2 - i) % net.n_ups;
            const float* uw = &net.ups_w[static_cast<size_t>(kidx) * net.ups_k];
            const float* pw = &net.pre_w[static_cast<size_t>(kidx) * net.pre_k];
            for (int a2 = 0; a2 < 4; ++a2)
                for (int b2 = a2; b2 < 4; ++b2) {
                    volatile float pu = uw[a2] * uw[b2], pp = pw[a2] * pw[b2];  // rounded to f32 like the kernels' own products
                    D.k2u[i][k2_index(a2, b2)] = pu; D.k2p[i][k2_index(a2, b2)] = pp;
                }
        }
        s.fdec_lds = fused_dec_lds_bytes(n_levels, C, D.n_conv, D.n_params, (b->opt_fused_dec == 2 && n_levels >= 5) ? 1 : 0);
        s.use_fused_dec = s.fdec_lds <= 160 * 1024;
        if (!s.use_fused_dec) syn_blob.resize(base);
        else p.at.fdec_params = base;
    }
}

// ---- 5. arena layout -------------------------------------------------------------------------------------------------
// The head of the arena - status block, payload words, integer networks, synthesis parameters - is what the host
// uploads: contiguous, staged in one pinned block, moved by ONE asynchronous copy (zeros included: the status words and
// the two payload words the decoder may read past the end).  Everything behind it is written by kernels before it is read.
void layout_arena(const ccd_batch* b, Slot& s, SlotPlan& p) {
    const ccd_cc_header& h = s.hdr;
    const std::vector<int>& lat_grids = p.lat_grids;
    const int n_levels = p.n_levels, H = h.img_size[0], W = h.img_size[1];
    Arena& A = s.arena;
    SlotLayout& at = p.at;
    at.status = A.reserve(512);
    at.words = A.reserve((p.n_words + 2) * 4);
    at.arm = A.reserve(p.blobs.arm.size() * 8);
    at.ifce = A.reserve(std::max<size_t>(p.blobs.ifce.size(), 1) * 8);
    size_t feat_px = 1;
    for (int g = 0; g < h.n_grids; ++g)
        if (h.input_features_ifce[g] > 0) {
            const int fg = (g == h.n_grids - 1) ? g : g + 1;
            feat_px = std::max(feat_px, static_cast<size_t>(h.grid_h[fg]) * h.grid_w[fg]);
        }
    const size_t dense_elems = static_cast<size_t>(s.dense_c) * s.dense_h * s.dense_w;
    size_t n_noise = 0, nstack_elems[2] = {1, 1};
    if (s.cr) {
        for (int i = 0; i < n_levels; ++i) {
            s.lvl_h.push_back(h.grid_h[lat_grids[i]]); s.lvl_w.push_back(h.grid_w[lat_grids[i]]);
            s.noise_off.push_back(n_noise);
            n_noise += static_cast<size_t>(s.lvl_h[i]) * s.lvl_w[i];
        }
        s.noise_off.push_back(n_noise);
        // intermediate stacks: level 1 holds n_levels-1 planes, level 2 n_levels-2 planes (the finest goes to dense)
        for (int k = 0; k < 2; ++k) {
            const int lv = k + 1;
            nstack_elems[k] = lv < n_levels ? static_cast<size_t>(n_levels - lv) * s.lvl_h[lv] * s.lvl_w[lv] : 1;
        }
    }
    size_t stack_b_elems = 1;
    if (n_levels >= 3) {
        const int g1 = lat_grids[1];
        stack_b_elems = static_cast<size_t>(n_levels - 1) * h.grid_h[g1] * h.grid_w[g1];
    }
    at.synp = A.reserve(p.syn_blob.size() * 4);
    at.head_bytes = A.total();
    at.lat.resize(h.n_grids);
    for (int g = 0; g < h.n_grids; ++g) at.lat[g] = A.reserve(static_cast<size_t>(h.grid_h[g]) * h.grid_w[g]);
    if (p.host_latents) at.head_bytes = A.total();  // given on the host: the grids are part of what is uploaded
    // int32 planes (generic kernel) or int16 planes + int32 side planes in the second half (pipelined kernel)
    if (s.given) feat_px = 1;  // no entropy kernel, no IFCE features
    at.feat_elems = feat_px * std::max(h.output_feature_ifce, 1);
    at.feat = A.reserve(at.feat_elems * 8);
    if (s.cr) {
        at.noise = A.reserve(n_noise * 4);
        for (int k = 0; k < 2; ++k) at.nstack[k] = A.reserve(nstack_elems[k] * 4);
    }
    const size_t plane_px = static_cast<size_t>(s.dense_h) * s.dense_w;
    // per-layer scratch of the generic synthesis path and the dense stacks of the unfused upsampling: only when that path runs
    const bool need_dense = !s.use_fused_dec || s.cr;  // (the noise planes are channels [n_levels, 2 n_levels) of the dense stack)
    const bool need_layers = !s.use_fused_dec && !s.use_fused_syn;
    // fused kernel behind the pyramid launch: the level-1 stack (channels 1 .. n_levels - 1 at level 1's size) is stack B
    s.fdec_pre = s.use_fused_dec && b->opt_fused_dec == 2 && n_levels >= 5;
    at.stack_a = A.reserve(need_dense ? dense_elems * 4 : 16);
    at.stack_b = A.reserve((need_dense || s.fdec_pre) ? stack_b_elems * 4 : 16);
    at.tmp0 = A.reserve(need_layers ? plane_px * p.max_c * 4 : 16);
    at.tmp1 = A.reserve(need_layers ? plane_px * p.max_c * 4 : 16);
    at.stab = A.reserve(need_layers ? plane_px * std::max(h.out_channels, 1) * 4 : 16);
    at.synout = A.reserve(plane_px * std::max(h.out_channels, 1) * 4);
    at.out = p.need_resize ? A.reserve(static_cast<size_t>(H) * W * h.out_channels * 4) : at.synout;
    // the three integer planes in one block (plane p at a 256-byte aligned offset): one copy takes them to the host
    const size_t sample_bytes = s.bitdepth == 8 ? 1 : 2;
    if (s.bitdepth) {
        size_t off = 0;
        for (int pl = 0; pl < 3; ++pl) {
            const bool chroma420 = (s.frame_data_type == 1 && pl > 0);
            s.plane_h[pl] = chroma420 ? H / 2 : H;
            s.plane_w[pl] = chroma420 ? W / 2 : W;
            s.plane_off[pl] = off;
            off += align256(static_cast<size_t>(s.plane_h[pl]) * s.plane_w[pl] * sample_bytes + 16);
        }
        s.planes_bytes = off;
        at.planes = A.reserve(off);
    }
}

// ---- 6. upload (inputs become resident in HBM here): the head, staged in pinned memory, one asynchronous copy on the
// device's upload stream; launches order themselves behind it with an event (ccd_batch_run_stage) --------------------
int upload_head(ccd_batch* b, Slot& s, const SlotPlan& p, const uint8_t* bytes_latent) {
    Arena& A = s.arena;
    const SlotLayout& at = p.at;
    auto fail = [&](int code) { A.release(); s.staging.drop(); return code; };
    if (!s.staging.get(b->device, BlockPool::kPinned, at.head_bytes)) return fail(CCD_ERR_NOMEM);
    char* st = s.staging.as<char>();
    std::memset(st + at.status, 0, 512);
    if (p.n_words) std::memcpy(st + at.words, bytes_latent, p.n_words * 4);
    std::memset(st + at.words + p.n_words * 4, 0, 8);
    if (!p.blobs.arm.empty()) std::memcpy(st + at.arm, p.blobs.arm.data(), p.blobs.arm.size() * 8);
    if (!p.blobs.ifce.empty()) std::memcpy(st + at.ifce, p.blobs.ifce.data(), p.blobs.ifce.size() * 8);
    if (!p.syn_blob.empty()) std::memcpy(st + at.synp, p.syn_blob.data(), p.syn_blob.size() * 4);
    if (p.host_latents)
        for (int g = 0; g < s.hdr.n_grids; ++g) std::memcpy(st + at.lat[g], p.host_latents[g], static_cast<size_t>(s.hdr.grid_h[g]) * s.hdr.grid_w[g]);
    if (hipMemcpyAsync(A.at<void>(0), st, at.head_bytes, hipMemcpyHostToDevice, b->up_stream) != hipSuccess) return fail(CCD_ERR_HIP);
    if (hipEventRecord(b->up_done, b->up_stream) != hipSuccess) return fail(CCD_ERR_HIP);
    b->uploads_unconfirmed = true;
    return CCD_OK;
}

// ---- 7. pointers.  Entropy stage description, then the upsampling levels (upsampling.py:486-498): coarsest -> finest ------
void bind_entropy_and_levels(const ccd_batch* b, Slot& s, const SlotPlan& p) {
    const ccd_cc_header& h = s.hdr;
    const Network& net = s.net;
    const std::vector<int>& lat_grids = p.lat_grids;
    const Arena& A = s.arena;
    const SlotLayout& at = p.at;
    EntropyParams& E = s.ep;
    std::memset(&E, 0, sizeof(E));
    E.words = A.at<uint32_t>(at.words); E.n_words = static_cast<uint32_t>(p.n_words);
    fill_entropy_model(h, net, p.blobs, E);
    for (int g = 0; g < h.n_grids; ++g) E.latent[g] = A.at<int8_t>(at.lat[g]);
    E.ring_rows = s.ring_rows;
    E.mfma = s.use_mfma ? std::min(std::max(b->opt_mfma_arm == 1 ? 23 : b->opt_mfma_arm, 1), 23) : 0;
    E.arm = A.at<int64_t>(at.arm);
    E.ifce = A.at<int64_t>(at.ifce);
    E.ifce_feat = A.at<int32_t>(at.feat);
    E.ifce_wide = A.at<int32_t>(at.feat) + at.feat_elems;
    E.feat_bits = b->opt_range_bits ? std::min(std::max(b->opt_range_bits, 8), 15) : 15;
    E.ifce_w32 = net.ifce_w32 ? 1 : 0;
    E.scale_table = b->d_scale_table;
    E.rcp_table = b->d_rcp_table;
    E.status = A.at<int32_t>(at.status);
    s.d_status = E.status;

    s.levels.clear();
    float* stack_a = A.at<float>(at.stack_a);
    float* stack_b = A.at<float>(at.stack_b);
    const int n_levels = p.n_levels, n_steps = n_levels - 1;
    const float* prev = nullptr;
    for (int step = 0; step < n_steps; ++step) {
        const int g_in = lat_grids[n_levels - 1 - step], g_out = lat_grids[n_levels - 2 - step];
        UpsampleLevel L;
        std::memset(&L, 0, sizeof(L));
        L.in_f32 = prev;
        L.in_i8 = (step == 0) ? E.latent[g_in] : nullptr;
        L.target = E.latent[g_out];
        L.out = ((n_steps - 1 - step) % 2 == 0) ? stack_a : stack_b;
        L.c_in = step + 1;
        L.h_in = h.grid_h[g_in]; L.w_in = h.grid_w[g_in];
        L.h_out = h.grid_h[g_out]; L.w_out = h.grid_w[g_out];
        L.ups_k = net.ups_k; L.pre_k = net.pre_k;
        const int kidx = step % net.n_ups;
        std::copy_n(&net.ups_w[static_cast<size_t>(kidx) * net.ups_k], net.ups_k, L.ups_w);
        std::copy_n(&net.pre_w[static_cast<size_t>(kidx) * net.pre_k], net.pre_k, L.pre_w);
        s.levels.push_back(L);
        prev = L.out;
    }
    s.d_dense = stack_a;
}

// ---- ... the buffers of the float stages, the SynthFused and FusedDec descriptors, the pyramid launch's descriptor --------
void bind_float_path(const ccd_batch* b, Slot& s, const SlotPlan& p) {
    const ccd_cc_header& h = s.hdr;
    const std::vector<int>& lat_grids = p.lat_grids;
    const Arena& A = s.arena;
    const SlotLayout& at = p.at;
    const EntropyParams& E = s.ep;
    const int n_levels = p.n_levels, bitdepth = s.bitdepth, frame_data_type = s.frame_data_type;
    const bool need_resize = p.need_resize;
    float* stack_b = A.at<float>(at.stack_b);
    if (s.cr) {
        s.d_noise = A.at<float>(at.noise);
        s.d_nstack[0] = A.at<float>(at.nstack[0]); s.d_nstack[1] = A.at<float>(at.nstack[1]);
    }
    s.d_syn_params = A.at<float>(at.synp);
    s.d_tmp[0] = A.at<float>(at.tmp0); s.d_tmp[1] = A.at<float>(at.tmp1);
    s.d_stab = A.at<float>(at.stab);
    s.d_syn_out = A.at<float>(at.synout);
    s.d_out = A.at<float>(at.out);
    for (int pl = 0; pl < 3; ++pl) s.d_plane[pl] = bitdepth ? A.at<void>(at.planes + s.plane_off[pl]) : nullptr;
    if (s.use_fused_syn) {
        SynthFused& F = s.fused;
        F.dense = s.d_dense; F.params = s.d_syn_params; F.h = s.dense_h; F.w = s.dense_w;
        F.bitdepth = bitdepth ? bitdepth : 8;
        // integer samples straight from the synthesis kernel for RGB / 4:4:4 frames at full resolution
        F.write_planes = (bitdepth != 0 && frame_data_type != 1 && !need_resize) ? 1 : 0;
        F.out = s.d_syn_out;
        for (int p = 0; p < 3; ++p) F.plane[p] = s.d_plane[p];
    }

    if (s.use_fused_dec) {
        FusedDec& D = s.fdec;
        D.params = s.d_syn_params + at.fdec_params;
        for (int i = 0; i < n_levels; ++i) { D.lat[i] = E.latent[lat_grids[i]]; D.lh[i] = h.grid_h[lat_grids[i]]; D.lw[i] = h.grid_w[lat_grids[i]]; }
        D.bitdepth = bitdepth ? bitdepth : 8;
        // integer samples straight from the kernel's epilogue: 1 = three full-size planes (rgb / yuv444), 2 = yuv420 (luma +
        // the 2 x 2 means of the chroma quads)
        D.write_planes = (bitdepth != 0 && !need_resize) ? (frame_data_type == 1 ? (h.out_channels >= 3 ? 2 : 0) : 1) : 0;
        // float samples: always when nothing else is produced (or a later stage reads them); otherwise by CCD_OPT_KEEP_FLOAT
        D.out = (!D.write_planes || b->opt_keep_float) ? s.d_syn_out : nullptr;
        for (int p = 0; p < 3; ++p) D.plane[p] = s.d_plane[p];
        D.l1 = nullptr;
        D.noise = s.cr ? s.d_dense + static_cast<size_t>(n_levels) * s.dense_h * s.dense_w : nullptr;
        if (s.fdec_pre) {
            // the pyramid launch's descriptor: this frame's levels 1 .. n - 1 as levels 0 .. n - 2, 64 x 32 tiles without margin,
            // output = the level-1 stack the main launch's tiles load
            FusedDec& Y = s.fpyr;
            std::memset(&Y, 0, sizeof(Y));
            Y.n_lv = n_levels - 1;
            for (int i = 0; i + 1 < n_levels; ++i) {
                Y.lat[i] = D.lat[i + 1]; Y.lh[i] = D.lh[i + 1]; Y.lw[i] = D.lw[i + 1];
                std::memcpy(Y.k2u[i], D.k2u[i + 1], sizeof(Y.k2u[i]));
                std::memcpy(Y.k2p[i], D.k2p[i + 1], sizeof(Y.k2p[i]));
            }
            Y.h = Y.lh[0]; Y.w = Y.lw[0]; Y.c = 2; Y.bitdepth = 8;
            Y.tiles_x = (Y.w + 63) / 64; Y.tiles_y = (Y.h + 31) / 32;
            Y.out = stack_b;
            D.l1 = stack_b;
        }
        s.levels.clear();  // no unfused pyramid steps for this slot
        s.use_fused_syn = false;
    }
}
}  // namespace

// ---- 8. what ccd_batch_add and ccd_batch_add_latents share once the slot is parsed: plan, lay out, upload, bind ------------
static int place_slot(ccd_batch* b, std::unique_ptr<Slot> sp, SlotPlan& p, const uint8_t* bytes_latent) {
    Slot& s = *sp;
    int rc = CCD_OK;
    if (s.given) pack_int_networks(s.hdr, s.net, p.blobs);  // (the arena keeps its layout; no entropy kernel is chosen)
    else rc = choose_entropy_kernel(b, s, p);
    if (rc >= 0) rc = float_geometry(s, p);
    if (rc < 0) return rc;
    layout_synthesis(b, s, p);
    layout_fused_dec(b, s, p);
    layout_arena(b, s, p);
    HIP_TRY(hipSetDevice(b->device));
    rc = s.arena.commit(b->device);
    if (rc >= 0) rc = upload_head(b, s, p, bytes_latent);
    if (rc < 0) return rc;
    bind_entropy_and_levels(b, s, p);
    bind_float_path(b, s, p);
    if (!s.given) {
        if (s.use_pipe) b->lds_pipe = std::max(b->lds_pipe, s.lds_pipe);
        else b->lds_generic = std::max(b->lds_generic, s.lds_generic);
    }
    b->slots.push_back(std::move(sp));
    return static_cast<int>(b->slots.size()) - 1;
}

extern "C" int ccd_batch_add(ccd_batch* b, const uint8_t* cc_header, size_t n_hdr, const uint8_t* bytes_nn, size_t n_nn,
                             const uint8_t* bytes_latent, size_t n_lat, int bitdepth, int frame_data_type) {
    if (!b || !cc_header || !bytes_nn || (!bytes_latent && n_lat)) return CCD_ERR_ARG;
    if (bitdepth != 0 && (bitdepth < 8 || bitdepth > 16)) return CCD_ERR_ARG;
    HIP_TRY(hipSetDevice(b->device));
    std::unique_ptr<Slot> sp(new (std::nothrow) Slot());
    if (!sp) return CCD_ERR_NOMEM;
    SlotPlan p;
    p.n_words = n_lat / 4;
    const int rc = parse_slot(*sp, cc_header, n_hdr, bytes_nn, n_nn, n_lat, bitdepth, frame_data_type);
    if (rc < 0) return rc;
    return place_slot(b, std::move(sp), p, bytes_latent);
}

extern "C" int ccd_batch_add_latents(ccd_batch* b, const ccd_cc_header* arch, const uint8_t* bytes_nn, size_t n_nn,
                                     const int8_t* const* latents, int on_device, int bitdepth, int frame_data_type) {
    if (!b || !arch || !bytes_nn || !latents) return CCD_ERR_ARG;
    if (bitdepth != 0 && (bitdepth < 8 || bitdepth > 16)) return CCD_ERR_ARG;
    std::unique_ptr<Slot> sp(new (std::nothrow) Slot());
    if (!sp) return CCD_ERR_NOMEM;
    Slot& s = *sp;
    // ---- everything the host can refuse, before the device is touched ----
    std::vector<uint8_t> hb;  // the header a coded slot would have brought: the transmitted fields, serialised with an empty payload
    int rc = rederive_cc_header(*arch, n_nn, &s.hdr, &hb);
    if (rc >= 0) rc = parse_slot(s, hb.data(), hb.size(), bytes_nn, n_nn, 0, bitdepth, frame_data_type);
    if (rc < 0) return rc;
    const ccd_cc_header& h = s.hdr;
    if (h.n_symbols < 0 || h.n_symbols > 0x7fffffff) return CCD_ERR_UNSUPPORTED;  // (a segment's length is 32 bits)
    for (int g = 0; g < h.n_grids; ++g) if (!latents[g]) return CCD_ERR_ARG;
    SlotPlan p;
    s.given = true;
    s.given_device = on_device != 0;
    if (on_device) {
        for (int g = 0; g < h.n_grids; ++g) s.given_src[g] = latents[g];
    } else {
        for (int g = 0; g < h.n_grids; ++g) {
            const size_t cnt = static_cast<size_t>(h.grid_h[g]) * h.grid_w[g];
            for (size_t i = 0; i < cnt; ++i)
                if (latents[g][i] < kAcLo || latents[g][i] > kAcLo + kAlphabet - 1) return CCD_ERR_VALUE;
        }
        p.host_latents = latents;
    }
    return place_slot(b, std::move(sp), p, nullptr);
}

// Chain groups of a batch (pure: ccd_debug_chain_groups exposes it to the CPU tests).  est[i]: expected chain of slot i; inst[i]: its
// kernel instantiation (0 .. k - 1; -1: the generic kernel's launch); n_conc: streams that really run at once; n_cu: CUs of the
// device.  cg[i] = 0 for the slots within 3 % of the batch's longest chain, 1 within 20 %, 2 for the rest - capped so that
// (a) instantiations x groups <= n_conc: a launch per group only helps on a stream of its own;
// (b) every workgroup still finds a CU at once.  A stream's workgroup owns a CU (139 KB of LDS) and the hardware deals the
//     workgroups of ONE launch out to the 8 XCDs round-robin: two launches of 63 + 193 workgroups put 8 + 25 on one 32-CU XCD, the
//     33rd waits for a whole chain - 68 ms instead of 36.6 (profiles/r06/streams_in_flight_overlap_before_xcd_rule.txt; a single
//     launch of 256 deals 32 to each): sum over launches of ceil(n / 8) <= CUs / 8 - else the group boundaries are moved to
//     multiples of 8 streams (c, below), else fewer groups.
static void plan_chain_groups(const double* est, const int* inst, int n, int n_conc, int n_cu, int* cg) {
    constexpr int kXcd = 8;  // gfx950
    double est_max = 0.0;
    int n_inst = 0, n_generic = 0;
    for (int i = 0; i < n; ++i) {
        if (inst[i] < 0) { ++n_generic; continue; }
        est_max = std::max(est_max, est[i]);
        n_inst = std::max(n_inst, inst[i] + 1);
    }
    int max_cg = std::max(1, std::min(3, n_conc / std::max(1, n_inst)));
    const auto fits = [&](int groups) {
        int per_xcd = (n_generic + kXcd - 1) / kXcd;
        for (int k = 0; k < n_inst; ++k)
            for (int g = 0; g < groups; ++g) {
                int cnt = 0;
                for (int i = 0; i < n; ++i) cnt += (inst[i] == k && cg[i] == g) ? 1 : 0;
                per_xcd += (cnt + kXcd - 1) / kXcd;
            }
        return per_xcd <= n_cu / kXcd;
    };
    for (; max_cg >= 1; --max_cg) {
        for (int i = 0; i < n; ++i) {
            const int c = est[i] >= 0.97 * est_max ? 0 : (est[i] >= 0.80 * est_max ? 1 : 2);
            cg[i] = inst[i] < 0 ? 0 : std::min(c, max_cg - 1);
        }
        if (max_cg == 1 || fits(max_cg)) break;
        // (c) a nearly full chip: the same split with every group boundary moved to a multiple of 8 streams - the slowest streams of
        //     the next group join the slower one (their frames are synthesised a little later, nothing else changes) - deals whole
        //     rounds to the XCDs: 63 + 193 becomes 64 + 192 = 8 + 24 per XCD
        for (int k = 0; k < n_inst; ++k) {
            std::vector<int> idx;
            for (int i = 0; i < n; ++i) if (inst[i] == k) idx.push_back(i);
            std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return cg[x] != cg[y] ? cg[x] < cg[y] : est[x] > est[y]; });
            int bound = 0, prev = 0;
            for (int g = 0; g + 1 < max_cg; ++g) {
                for (int i : idx) bound += cg[i] == g ? 1 : 0;
                const int rounded = std::min(static_cast<int>(idx.size()), std::max(prev, (bound + kXcd - 1) / kXcd * kXcd));
                for (int r = prev; r < rounded; ++r) cg[idx[r]] = g;
                prev = rounded;
            }
            for (int r = prev; r < static_cast<int>(idx.size()); ++r) cg[idx[r]] = max_cg - 1;
        }
        if (fits(max_cg)) break;
    }
}

// Expected length of a slot's serial chain in decoder ticks (only the ORDER and rough ratios matter: it decides which streams
// share an entropy launch).  Per grid ~120 ticks per symbol + ~1.8 k per step of the coding order (ccd_wavefront.hpp):
// profiles/r06/prof_grids_base.txt - a portrait Kodak stream comes out 1.09 x a landscape one (measured 1.06).
static double chain_estimate(const EntropyParams& ep) {
    double t = 0.0;
    for (int g = 0; g < ep.n_grids; ++g) {
        const int h = ep.grid_h[g], w = ep.grid_w[g];
        t += 120.0 * h * w + 1800.0 * wf_n_steps(h, w);
    }
    return t;
}

namespace {
struct Work { int32_t frame, tile_first, tile_count, pad; };
// Host images of the tables the launches of a batch read, in the order they are packed into the one device block.
struct LaunchTables {
    std::vector<EntropyParams> params;
    std::vector<int> params_slot;  // slot of params[k]: its status words are words [64 slot, 64 slot + 64) of the batch's status array
    std::vector<SynthFused> fused;
    std::vector<FusedDec> frames, pyr_frames;
    std::vector<Work> work, pyr_work;
    std::vector<UpsampleLevel> levels;
    std::vector<uint32_t> zmap;
    std::vector<IngestSeg> ingest;
    std::vector<uint32_t> ingest_prefix;  // [segments + 1]
};

// Entropy launches.  The pipelined kernel is instantiated per input width nv = ceil(dim / 4): one launch per width.
    // ---- chain groups (r06).  A stream is one serial chain on one CU and a launch ends with its slowest stream; the float path of
    // a frame only needs THAT frame's latents.  So the slots of an instantiation are split by expected chain length into up to three
    // launches - the streams within 3 % of the batch's longest chain, those within 20 %, the rest - and ccd_batch_run puts each
    // launch's pyramid + fused launches directly behind it on its own stream: the float stage of the streams that finish early
    // hides behind the longest chains (kodak24: 18 landscape pictures are done 2 ms before the 6 portrait ones).  At most ~4
    // launches per batch: HIP streams share a handful of hardware queues.
void plan_entropy_groups(ccd_batch* b, LaunchTables& t) {
    const int n = static_cast<int>(b->slots.size());
    std::vector<EntropyParams>& host = t.params;
    std::vector<int>& host_slot = t.params_slot;
    b->pipe_groups.clear();
    std::vector<double> est(n, 0.0);
    std::vector<int> cg_of(n, 0), inst_of(n, -1);
    {
        // the slots whose latents are range-coded: a slot with GIVEN latents belongs to no entropy launch and is not planned for
        std::vector<int> coded;
        std::vector<std::array<int, 3>> insts;
        for (int i = 0; i < n; ++i) {
            const Slot& sl = *b->slots[i];
            if (sl.given) continue;
            coded.push_back(i);
            est[i] = chain_estimate(sl.ep);
            if (!sl.use_pipe) continue;  // (-1: the generic launch)
            const std::array<int, 3> key{(sl.ep.dim + 3) / 4, sl.use_mfma ? 2 : (sl.use_dyn ? 1 : 0), sl.fixed_shape};
            auto it = std::find(insts.begin(), insts.end(), key);
            inst_of[i] = static_cast<int>(it - insts.begin());
            if (it == insts.end()) insts.push_back(key);
        }
        // as many launches as streams really run at once (DeviceShared::n_conc, measured), shared between the instantiations
        int n_conc = 1, n_cu = 256;
        { DeviceShared* shd = nullptr; if (device_shared(b->device, &shd) >= 0) { n_conc = shd->n_conc; n_cu = shd->n_cu; } }
        const int nc = static_cast<int>(coded.size());
        std::vector<double> est_c(nc);
        std::vector<int> inst_c(nc), cg_c(nc, 0);
        for (int k = 0; k < nc; ++k) { est_c[k] = est[coded[k]]; inst_c[k] = inst_of[coded[k]]; }
        plan_chain_groups(est_c.data(), inst_c.data(), nc, b->opt_overlap ? n_conc : 1, n_cu, cg_c.data());
        for (int k = 0; k < nc; ++k) cg_of[coded[k]] = cg_c[k];
    }
    for (int nv = 1; nv <= 8; ++nv)
        for (int var = 0; var < 3; ++var)  // vector ALU without / with the device check of the features, matrix cores
            for (int shape = 0; shape < 2; ++shape)  // run-time ARM shape / the compile-time instantiation of the HOP shape
                for (int cg = 0; cg < 3; ++cg) {
                    const int mf = var == 2 ? 1 : 0, dyn = var == 1 ? 1 : 0;
                    const int first = static_cast<int>(host.size());
                    size_t lds = 0;
                    double est_g = 0.0;
                    for (int i = 0; i < n; ++i) {
                        Slot& sl = *b->slots[i];
                        if (sl.use_pipe && (sl.ep.dim + 3) / 4 == nv && (sl.use_mfma ? 1 : 0) == mf && (sl.use_dyn ? 1 : 0) == dyn && sl.fixed_shape == shape && cg_of[i] == cg) {
                            host.push_back(sl.ep); host_slot.push_back(i); lds = std::max(lds, sl.lds_pipe);
                            est_g = std::max(est_g, est[i]);
                            sl.lg = static_cast<int>(b->pipe_groups.size());
                        }
                    }
                    if (static_cast<int>(host.size()) > first) b->pipe_groups.push_back({nv, mf, dyn, shape, cg, first, static_cast<int>(host.size()) - first, lds, est_g});
                }
    for (int i = 0; i < n; ++i) {
        Slot& sl = *b->slots[i];
        if (!sl.use_pipe) sl.lg = -1;
        // float launches keyed by the entropy launch they follow - only worth it (and only done) when there are several launches
        sl.fl = (b->opt_overlap && sl.use_pipe) ? sl.lg : -1;
    }
    b->n_pipe = static_cast<int>(host.size());
    for (int i = 0; i < n; ++i) if (!b->slots[i]->use_pipe && !b->slots[i]->given) { host.push_back(b->slots[i]->ep); host_slot.push_back(i); }
    b->n_generic = static_cast<int>(host.size()) - b->n_pipe;
}

// the ingest launch (ccd_ingest.hip): a segment per grid of every slot whose latents are device pointers, and the first
// workgroup of each segment
void plan_ingest(ccd_batch* b, LaunchTables& t) {
    uint32_t blocks = 0;
    for (size_t i = 0; i < b->slots.size(); ++i) {
        const Slot& s = *b->slots[i];
        if (!s.given_device) continue;
        for (int g = 0; g < s.hdr.n_grids; ++g) {
            const uint32_t cnt = static_cast<uint32_t>(s.hdr.grid_h[g]) * static_cast<uint32_t>(s.hdr.grid_w[g]);
            if (!cnt) continue;
            t.ingest.push_back({s.given_src[g], s.ep.latent[g], cnt, static_cast<int32_t>(i)});
            t.ingest_prefix.push_back(blocks);
            blocks += (cnt + kIngestChunk - 1) / kIngestChunk;
        }
    }
    if (!t.ingest.empty()) t.ingest_prefix.push_back(blocks);
    b->n_ingest = static_cast<int>(t.ingest.size());
    b->n_ingest_blocks = blocks;
}

// fused synthesis: one launch per (CP, C) group over all of its frames
void plan_fused_syn_groups(ccd_batch* b, LaunchTables& t) {
    const int n = static_cast<int>(b->slots.size());
    std::vector<SynthFused>& fused = t.fused;
    b->fused_groups.clear();
    for (int i = 0; i < n; ++i) {
        const Slot& s = *b->slots[i];
        if (!s.use_fused_syn) continue;
        const int cp = (s.fused.c_in + 3) / 4;
        bool placed = false;
        for (auto& g : b->fused_groups) placed = placed || (g.cp == cp && g.c == s.fused.c);
        if (!placed) b->fused_groups.push_back({cp, s.fused.c, s.fused.c_in, 0, 0, 0, 0});
    }
    for (auto& g : b->fused_groups) {
        g.first = static_cast<int>(fused.size());
        for (int i = 0; i < n; ++i) {
            const Slot& s = *b->slots[i];
            if (!s.use_fused_syn || (s.fused.c_in + 3) / 4 != g.cp || s.fused.c != g.c) continue;
            int tx = 0, ty = 0;
            syn_fused_tiles(s.fused.h, s.fused.w, s.fused.halo, &tx, &ty);
            g.max_tx = std::max(g.max_tx, tx); g.max_ty = std::max(g.max_ty, ty);
            fused.push_back(s.fused);
            ++g.n;
        }
    }
}

// Appends one launch's frames (the descriptors `pick` returns, in slot order) and its work list: a workgroup takes a run of
// `per_wg` tiles of one frame.  Returns the number of work items (0: no frame picked, nothing appended).
// XCD-aware order of one launch's work list (r06).  The hardware deals the workgroups of a launch out to the 8 XCDs round-robin
// (workgroup i -> XCD i mod 8, tools/ubench/queues.hip prints it) and every XCD has its own L2: with the work items in raster
// order, neighbouring tiles - which share the halo rows / columns of the level-1 stack and the latent tile - always sat on
// DIFFERENT XCDs and each fetched the shared cache lines from HBM for itself (main launch of the fused float path: 165 MB
// fetched per 24 Kodak frames for ~70 MB of stack + latents, profiles/r05/kodak24_pmc_traffic.json).  Here item j of the natural
// order goes to a workgroup of XCD x = the eighth of the list it lies in: every XCD walks ONE contiguous run of tiles.
template <typename Pick>
int append_tile_runs(const ccd_batch* b, Pick pick, std::vector<FusedDec>& frames, std::vector<Work>& work) {
    const size_t first_frame = frames.size(), first = work.size();
    long total_tiles = 0;
    for (const auto& sp : b->slots) if (const FusedDec* d = pick(*sp)) total_tiles += static_cast<long>(d->tiles_x) * d->tiles_y;
    if (!total_tiles) return 0;
    // ~8 workgroups per CU keep the tail short; a run of tiles amortises the parameter staging
    const int per_wg = static_cast<int>(std::min<long>(8, std::max<long>(1, (total_tiles + 2047) / 2048)));
    for (const auto& sp : b->slots) {
        const FusedDec* d = pick(*sp);
        if (!d) continue;
        const int f = static_cast<int>(frames.size() - first_frame);
        frames.push_back(*d);
        const int nt = d->tiles_x * d->tiles_y;
        for (int t0 = 0; t0 < nt; t0 += per_wg) work.push_back({f, t0, std::min(per_wg, nt - t0), 0});
    }
    constexpr size_t kXcd = 8;
    const size_t n = work.size() - first;
    if (n >= 2 * kXcd && !std::getenv("CCD_NO_XCD_ORDER")) {
        const std::vector<Work> nat(work.begin() + static_cast<std::ptrdiff_t>(first), work.end());
        size_t start = 0;
        for (size_t x = 0; x < kXcd; ++x) {
            const size_t cnt = (n - x + kXcd - 1) / kXcd;  // workgroups x, x + 8, ... of the launch
            for (size_t k = 0; k < cnt; ++k) work[first + x + kXcd * k] = nat[start + k];
            start += cnt;
        }
    }
    return static_cast<int>(n);
}

// What the frames of one fused-decode launch share.
struct FdecKey {
    int n_lv, c, pre, cr, fl;
    bool operator==(const FdecKey& o) const { return n_lv == o.n_lv && c == o.c && pre == o.pre && cr == o.cr && fl == o.fl; }
};
FdecKey fdec_key(const Slot& s) { return {s.fdec.n_lv, s.fdec.c, s.fdec_pre ? 1 : 0, s.cr ? 1 : 0, s.fl}; }

// fused float path: frames grouped by (levels, channels, pyramid launch or not, common randomness, entropy launch they follow)
void plan_fdec_groups(ccd_batch* b, LaunchTables& t) {
    b->fdec_groups.clear();
    for (const auto& sp : b->slots) {
        if (!sp->use_fused_dec) continue;
        const FdecKey k = fdec_key(*sp);
        bool placed = false;
        for (auto& g : b->fdec_groups) placed = placed || FdecKey{g.c_in, g.c, g.pre, g.cr, g.fl} == k;
        if (!placed) b->fdec_groups.push_back({k.n_lv, k.c, k.pre, k.cr, k.fl, 0, 0, 0, 0});
    }
    for (auto& g : b->fdec_groups) {
        const FdecKey k{g.c_in, g.c, g.pre, g.cr, g.fl};
        g.first_frame = static_cast<int>(t.frames.size());
        g.first_work = static_cast<int>(t.work.size());
        for (const auto& sp : b->slots) if (sp->use_fused_dec && fdec_key(*sp) == k) g.lds = std::max(g.lds, sp->fdec_lds);
        g.n_work = append_tile_runs(b, [&](const Slot& s) { return s.use_fused_dec && fdec_key(s) == k ? &s.fdec : nullptr; }, t.frames, t.work);
    }
}

// pyramid launches of the kFdPre slots: one per number of levels and entropy launch they follow
void plan_pyr_groups(ccd_batch* b, LaunchTables& t) {
    b->pyr_groups.clear();
    for (int lv = 2; lv < kFdMaxLevels; ++lv)
        for (int fl = -1; fl < static_cast<int>(b->pipe_groups.size()); ++fl) {
            ccd_batch::PyrGroup g{lv, fl, static_cast<int>(t.pyr_frames.size()), static_cast<int>(t.pyr_work.size()), 0, fused_pyr_lds_bytes(lv + 1)};
            g.n_work = append_tile_runs(b, [&](const Slot& s) { return s.fdec_pre && s.fpyr.n_lv == lv && s.fl == fl ? &s.fpyr : nullptr; }, t.pyr_frames, t.pyr_work);
            if (g.n_work) b->pyr_groups.push_back(g);
        }
}

// upsampling steps: step k (k-th from the coarsest level) of all slots together
int plan_ups_steps(ccd_batch* b, LaunchTables& t) {
    const int n = static_cast<int>(b->slots.size());
    std::vector<UpsampleLevel>& levels = t.levels;
    std::vector<uint32_t>& zmap = t.zmap;
    b->ups_steps.clear();
    size_t max_steps = 0;
    for (int i = 0; i < n; ++i) max_steps = std::max(max_steps, b->slots[i]->levels.size());
    for (size_t k = 0; k < max_steps; ++k) {
        ccd_batch::UpsStep st{static_cast<int>(zmap.size()), 0, 0, 0};
        for (int i = 0; i < n; ++i) {
            const Slot& s = *b->slots[i];
            if (k >= s.levels.size()) continue;
            if (levels.size() >= 65535) return CCD_ERR_UNSUPPORTED;
            const uint32_t li = static_cast<uint32_t>(levels.size());
            levels.push_back(s.levels[k]);
            // group 0 = pre-concat conv; group g >= 1 = transposed conv of input channels 2g-2, 2g-1
            for (int grp = 0; grp <= (s.levels[k].c_in + 1) / 2; ++grp) zmap.push_back((li << 16) | static_cast<uint32_t>(grp));
            st.max_w = std::max(st.max_w, static_cast<int>(s.levels[k].w_out));
            st.max_h = std::max(st.max_h, static_cast<int>(s.levels[k].h_out));
        }
        st.n_z = static_cast<int>(zmap.size()) - st.first_z;
        b->ups_steps.push_back(st);
    }
    return CCD_OK;
}

// ---- one pooled device block for every table and the status words of all slots, filled by ONE copy from ONE pinned block
int pack_and_upload(ccd_batch* b, LaunchTables& t, hipStream_t st) {
    const int n = static_cast<int>(b->slots.size());
    const size_t o_params = 0;
    const size_t o_fusedt = o_params + align256(sizeof(EntropyParams) * std::max(n, 1));
    const size_t o_fdec = o_fusedt + align256(sizeof(SynthFused) * std::max<size_t>(t.fused.size(), 1));
    const size_t o_work = o_fdec + align256(sizeof(FusedDec) * std::max<size_t>(t.frames.size(), 1));
    const size_t o_levels = o_work + align256(sizeof(Work) * std::max<size_t>(t.work.size(), 1));
    const size_t o_zmap = o_levels + align256(sizeof(UpsampleLevel) * std::max<size_t>(t.levels.size(), 1));
    const size_t o_pyr = o_zmap + align256(sizeof(uint32_t) * std::max<size_t>(t.zmap.size(), 1));
    const size_t o_pyrw = o_pyr + align256(sizeof(FusedDec) * std::max<size_t>(t.pyr_frames.size(), 1));
    const size_t o_stat = o_pyrw + align256(sizeof(Work) * std::max<size_t>(t.pyr_work.size(), 1));
    // (the ingest tables come last and only exist with device-latent slots: every other batch keeps the layout it had)
    const size_t o_ingest = o_stat + align256(static_cast<size_t>(std::max(n, 1)) * 64 * sizeof(int32_t));
    const size_t o_ingestp = o_ingest + (t.ingest.empty() ? 0 : align256(sizeof(IngestSeg) * t.ingest.size()));
    const size_t total = o_ingestp + (t.ingest.empty() ? 0 : align256(sizeof(uint32_t) * t.ingest_prefix.size()));
    // the previous tables may still be read by launches in flight on the caller's stream (a batch that grew between runs)
    if (b->tables.p && b->drain() < 0) return CCD_ERR_HIP;
    if (!b->tables.get(b->device, BlockPool::kDevice, total) || !b->tables_staging.get(b->device, BlockPool::kPinned, total) ||
        !b->status_host.get(b->device, BlockPool::kPinned, static_cast<size_t>(std::max(n, 1)) * 64 * sizeof(int32_t)))
        return CCD_ERR_NOMEM;
    char* dev = b->tables.as<char>();
    char* stg = b->tables_staging.as<char>();
    b->d_params = reinterpret_cast<EntropyParams*>(dev + o_params);
    b->d_fused = reinterpret_cast<SynthFused*>(dev + o_fusedt);
    b->d_fdec = reinterpret_cast<FusedDec*>(dev + o_fdec);
    b->d_fdec_work = dev + o_work;
    b->d_levels = reinterpret_cast<UpsampleLevel*>(dev + o_levels);
    b->d_zmap = reinterpret_cast<uint32_t*>(dev + o_zmap);
    b->d_pyr = reinterpret_cast<FusedDec*>(dev + o_pyr);
    b->d_pyr_work = dev + o_pyrw;
    b->d_status_all = reinterpret_cast<int32_t*>(dev + o_stat);
    b->d_ingest = reinterpret_cast<IngestSeg*>(dev + o_ingest);
    b->d_ingest_prefix = reinterpret_cast<uint32_t*>(dev + o_ingestp);
    for (size_t k = 0; k < t.params.size(); ++k) t.params[k].status = b->d_status_all + static_cast<size_t>(t.params_slot[k]) * 64;
    for (int i = 0; i < n; ++i) b->slots[i]->d_status = b->d_status_all + static_cast<size_t>(i) * 64;
    const auto put = [&](size_t off, const auto& v) { if (!v.empty()) std::memcpy(stg + off, v.data(), sizeof(v[0]) * v.size()); };
    put(o_params, t.params); put(o_fusedt, t.fused); put(o_fdec, t.frames); put(o_work, t.work);
    put(o_levels, t.levels); put(o_zmap, t.zmap); put(o_pyr, t.pyr_frames); put(o_pyrw, t.pyr_work);
    std::memset(stg + o_stat, 0, o_ingest - o_stat);  // every status word starts as CCD_OK: a given slot's is never written unless a latent is refused
    put(o_ingest, t.ingest); put(o_ingestp, t.ingest_prefix);
    HIP_TRY(hipMemcpyAsync(dev, stg, total, hipMemcpyHostToDevice, st));
    // a later run on ANOTHER stream (ccd_batch_prepare on one, ccd_batch_run on the next) orders itself behind this copy
    if (!b->params_up) HIP_TRY(hipEventCreateWithFlags(&b->params_up, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(b->params_up, st));
    b->params_stream = st;
    b->n_params_uploaded = n;
    return CCD_OK;
}
}  // namespace

int ccd::build_launch_tables(ccd_batch* b, hipStream_t st) {
    if (b->n_params_uploaded == static_cast<int>(b->slots.size()) && !b->regroup) return CCD_OK;
    b->regroup = false;
    LaunchTables t;
    plan_entropy_groups(b, t);
    plan_ingest(b, t);
    plan_fused_syn_groups(b, t);
    plan_fdec_groups(b, t);
    plan_pyr_groups(b, t);
    const int rc = plan_ups_steps(b, t);
    return rc < 0 ? rc : pack_and_upload(b, t, st);
}

extern "C" int ccd_debug_chain_groups(const double* est, const int32_t* inst, int n, int n_conc, int n_cu, int32_t* cg) {
    if (!est || !inst || !cg || n < 0 || n_conc < 1 || n_cu < 8) return CCD_ERR_ARG;
    plan_chain_groups(est, inst, n, n_conc, n_cu, cg);
    int groups = 0;
    for (int i = 0; i < n; ++i) groups = std::max(groups, cg[i] + 1);
    return groups;
}
