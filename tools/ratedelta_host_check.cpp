// ratedelta_host_check.cpp - the planning of the ARM and the IFCE parameter tables (cool_chic_amd/csrc/ccd_ratedelta_plan.hpp,
// DESIGN.md sections 4.20 and 4.21) against decode_network, as a stand-alone CPU program: meant to be built with
// -fsanitize=address,undefined together with the two host sources it exercises, host code only (no device code is compiled, no
// device is needed, and the sanitizers are never asked of an offload target):
//
//   hipcc --offload-host-only -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/ratedelta_host_check.cpp cool_chic_amd/csrc/ccd_format.cpp cool_chic_amd/csrc/ccd_writer.cpp -o ratedelta_host_check
//   ./ratedelta_host_check tests/golden/*.cool
//
// Every cool-chic of every stream, and the shapes of tests/arm_layouts.py made from the first cool-chic's architecture with seeded
// integers (for the ARM: ARM_SHAPES, PLACEMENT_SHAPES, TINY_SHAPES; for the IFCE: its placements and its shapes with IFCE features,
// at 18 x 65).  For every integer k of a network and both signs the plan is checked (range, no entry shared by two parameters,
// every entry some parameter's), then values[k] + s is encoded again (ccd_encode_network), decoded (decode_network), and the whole
// fixed-point ARM and ALL fixed-point IFCE blocks are compared with the base's: exactly the planned entry differs, by exactly the
// planned increment.  ARMs of more than 2 048 integers have the plan of every (k, s) checked and the decode within 8 parameters of
// every layer's first weight, of the first bias and of both ends: the whole program then takes about two minutes under the
// sanitizers.  Then the int32 edges (the first weight at 2^31 - 1, the last bias at -2^31) and the refusals.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../cool_chic_amd/csrc/ccd_format.hpp"
#include "../cool_chic_amd/csrc/ccd_ratedelta_plan.hpp"

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

using namespace ccd;

static std::vector<uint8_t> read_file(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    CHECK(f);
    std::vector<uint8_t> out;
    uint8_t buf[65536];
    for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;) out.insert(out.end(), buf, buf + n);
    std::fclose(f);
    return out;
}

// the fixed-point networks in the order the kernels read them (pack_int_networks): block 0 the ARM, block 1 + g the IFCE of
// grid g (w[fin][n_if], b[n_if]; empty without IFCE there)
using Decoded = std::vector<std::vector<int64_t>>;
static Decoded decoded(const ccd_cc_header& arch, const std::vector<int32_t>& ints) {
    ccd_cc_header h = arch;
    int32_t pad = -1;
    uint8_t* out = nullptr;
    const int64_t n = ccd_encode_network(&h, ints.data(), static_cast<int64_t>(ints.size()), &pad, &out);
    CHECK(n >= 0);
    h.nn_n_bytes = static_cast<int32_t>(n);
    h.nn_n_bit_pad = pad;
    Network net;
    CHECK(decode_network(h, out, static_cast<size_t>(n), net) == CCD_OK);
    std::free(out);
    Decoded d(1 + static_cast<size_t>(h.n_grids));
    auto append = [](std::vector<int64_t>& to, const std::vector<int64_t>& v) { to.insert(to.end(), v.begin(), v.end()); };
    for (const FixedLayer& L : net.arm.layers) { append(d[0], L.w); append(d[0], L.b); }
    append(d[0], net.arm.ws);
    append(d[0], net.arm.bs);
    for (int g = 0; g < h.n_grids; ++g) {
        if (net.ifce[static_cast<size_t>(g)].dim == 0) continue;
        const FixedLayer& L = net.ifce[static_cast<size_t>(g)].layers[0];
        append(d[1 + static_cast<size_t>(g)], L.w);
        append(d[1 + static_cast<size_t>(g)], L.b);
    }
    return d;
}

// ints[at] + sign (legal: it stays in int32) encoded again and decoded: of all blocks exactly entry `index` of `block` differs
// from the base's, by exactly mv.inc
static void check_decode(const ccd_cc_header& arch, std::vector<int32_t>& ints, size_t at, int sign, const Decoded& base, size_t block,
                         int64_t index, const RateDeltaMove& mv) {
    const int32_t keep = ints[at];
    ints[at] = keep + sign;
    const Decoded got = decoded(arch, ints);
    ints[at] = keep;
    CHECK(got.size() == base.size());
    for (size_t b = 0; b < base.size(); ++b) {
        CHECK(got[b].size() == base[b].size());
        for (size_t i = 0; i < base[b].size(); ++i) {
            const bool planned = b == block && static_cast<int64_t>(i) == index;
            CHECK(static_cast<uint64_t>(got[b][i]) == static_cast<uint64_t>(base[b][i]) + (planned ? static_cast<uint64_t>(mv.inc) : 0));
        }
    }
}

// what the two networks' plans share for candidate (k, sign) of the integer ints[at]: the move, its legality, and that no two
// parameters share an entry (`seen`: of the block the plan names)
static RateDeltaMove check_move(int rc_place, RateDeltaMove mv, int shift, int sign, int32_t value, int64_t index, std::vector<char>& seen) {
    CHECK(rc_place == CCD_OK && ratedelta_move(sign, value, shift, &mv) == CCD_OK);
    CHECK(index >= 0 && index < static_cast<int64_t>(seen.size()));
    const int64_t moved = static_cast<int64_t>(value) + sign;
    CHECK(mv.legal == (moved >= INT32_MIN && moved <= INT32_MAX));
    if (sign < 0) { CHECK(!seen[static_cast<size_t>(index)]); seen[static_cast<size_t>(index)] = 1; }
    return mv;
}

constexpr int64_t kWholeTable = 2048;
// first weight of layer l in STREAM order (l == n_layers: the stabiliser's)
static int64_t armdelta_layer_weights_first(const ArmDeltaShape& s, int l) {
    return l < s.n_layers ? static_cast<int64_t>(l) * s.dim * s.dim : static_cast<int64_t>(s.n_layers - 1) * s.dim * s.dim + 2 * s.dim;
}
// every (k, s) of one network's ARM; returns the number of candidates decoded
static long check_arm(const ccd_cc_header& arch, std::vector<int32_t> ints, const Decoded& base) {
    const ArmDeltaShape shape = armdelta_shape(arch);
    int64_t n_kind[8];
    CHECK(ccd_network_layout(&arch, n_kind) == CCD_OK);
    const int64_t n_arm = n_kind[0] + n_kind[1];
    CHECK(armdelta_count(shape) == n_arm && armdelta_n_weights(shape) == n_kind[0] && armdelta_n_biases(shape) == n_kind[1]);
    CHECK(static_cast<int64_t>(base[0].size()) == armdelta_layer_first(shape, shape.n_layers) + 2 * shape.dim + 2);
    std::vector<char> seen(base[0].size(), 0);
    long n = 0;
    // a network of more than kWholeTable integers: the plan of every (k, s) is checked, the decode only within 8 parameters of a
    // layer's first weight, of the first bias and of both ends (a decode re-reads the whole payload: 36 072 integers the largest)
    std::vector<int64_t> marks{0, n_kind[0], n_arm};
    for (int l = 1; l <= shape.n_layers; ++l) marks.push_back(armdelta_layer_weights_first(shape, l));
    auto near_mark = [&](int64_t k) {
        for (int64_t m : marks) if (k >= m - 8 && k < m + 8) return true;
        return false;
    };
    for (int64_t k = 0; k < n_arm; ++k)
        for (int sign = -1; sign <= 1; sign += 2) {
            RateDeltaMove mv{};
            int64_t index = -1;
            int shift = 0;
            const int rc = armdelta_place(shape, k, &mv, &index, &shift);
            mv = check_move(rc, mv, shift, sign, ints[static_cast<size_t>(k)], index, seen);
            CHECK(mv.at >= 0 && mv.at <= shape.n_layers && mv.out >= 0 && mv.out < (mv.at < shape.n_layers - 1 ? shape.dim : 2) &&
                  mv.in >= -1 && mv.in < shape.dim);
            CHECK(shape.stabiliser || mv.at < shape.n_layers);
            if (!mv.legal || (n_arm > kWholeTable && !near_mark(k))) continue;
            check_decode(arch, ints, static_cast<size_t>(k), sign, base, 0, index, mv);
            ++n;
        }
    if (shape.stabiliser) for (char s : seen) CHECK(s);  // every entry of the fixed-point ARM is some parameter's
    return n;
}

// every (k, s) of one network's IFCE; returns the number of candidates decoded
static long check_ifce(const ccd_cc_header& arch, std::vector<int32_t> ints, const Decoded& base) {
    const IfceDeltaShape shape = ifcedelta_shape(arch);
    int64_t n_kind[8];
    CHECK(ccd_network_layout(&arch, n_kind) == CCD_OK);
    const int64_t n_arm = n_kind[0] + n_kind[1], n_ifce = n_kind[2] + n_kind[3];
    CHECK(ifcedelta_count(shape) == n_ifce && ifcedelta_n_weights(shape) == n_kind[2] && ifcedelta_n_biases(shape) == n_kind[3]);
    if (n_ifce == 0) return 0;
    const int n_if = shape.n_ifce_out;
    std::vector<std::vector<char>> seen(static_cast<size_t>(shape.n_grids));
    for (int g = 0; g < shape.n_grids; ++g) {
        CHECK(static_cast<int64_t>(base[1 + static_cast<size_t>(g)].size()) == (shape.fin[g] > 0 ? static_cast<int64_t>(shape.fin[g] + 1) * n_if : 0));
        seen[static_cast<size_t>(g)].assign(base[1 + static_cast<size_t>(g)].size(), 0);
    }
    long n = 0;
    int last_grid_w = 0, last_grid_b = 0;
    for (int64_t k = 0; k < n_ifce; ++k)
        for (int sign = -1; sign <= 1; sign += 2) {
            RateDeltaMove mv{};
            int64_t index = -1;
            int shift = 0;
            const size_t at = static_cast<size_t>(n_arm + k);
            const int rc = ifcedelta_place(shape, k, &mv, &index, &shift);
            CHECK(rc == CCD_OK && mv.at >= 0 && mv.at < shape.n_grids && shape.fin[mv.at] > 0 && mv.out >= 0 && mv.out < n_if && mv.in >= -1 &&
                  mv.in < shape.fin[mv.at]);
            mv = check_move(rc, mv, shift, sign, ints[at], index, seen[static_cast<size_t>(mv.at)]);
            CHECK((mv.in < 0) == (k >= n_kind[2]));
            // stream order: the grids ascend inside the weights and inside the biases
            int& last = mv.in < 0 ? last_grid_b : last_grid_w;
            CHECK(mv.at >= last);
            last = mv.at;
            if (!mv.legal) continue;
            check_decode(arch, ints, at, sign, base, 1 + static_cast<size_t>(mv.at), index, mv);  // the ARM does not differ at all
            ++n;
        }
    for (const auto& grid : seen) for (char s : grid) CHECK(s);  // every IFCE entry is some parameter's
    return n;
}

static void check_refusals(const ccd_cc_header& arch) {
    RateDeltaMove mv{};
    int64_t index = 0;
    int shift = 0;
    // shared: the sign of a move, the modes and the one LDS limit
    CHECK(ratedelta_move(0, 0, 16, &mv) == CCD_ERR_ARG && ratedelta_move(2, 0, 16, &mv) == CCD_ERR_ARG);
    CHECK(ratedelta_path(0, -1) == CCD_ERR_ARG && ratedelta_path(0, 3) == CCD_ERR_ARG);
    for (const int64_t lds : {int64_t{0}, kArmDeltaMaxLds, kArmDeltaMaxLds + 1}) {
        const bool fits = lds <= kArmDeltaMaxLds;
        CHECK(ratedelta_path(lds, kArmDeltaGeneric) == kArmDeltaGeneric);
        CHECK(ratedelta_path(lds, kArmDeltaAuto) == (fits ? kArmDeltaIncremental : kArmDeltaGeneric));
        CHECK(ratedelta_path(lds, kArmDeltaIncremental) == (fits ? kArmDeltaIncremental : CCD_ERR_UNSUPPORTED));
    }
    // the ARM
    const ArmDeltaShape a = armdelta_shape(arch);
    CHECK(armdelta_place(a, -1, &mv, &index, &shift) == CCD_ERR_ARG && armdelta_place(a, armdelta_count(a), &mv, &index, &shift) == CCD_ERR_ARG);
    ArmDeltaShape wide = a;
    wide.dim = 71; wide.n_layers = 8;  // 10 x 71 columns of per-lane state: beyond the LDS
    CHECK(armdelta_incremental_lds(wide) > kArmDeltaMaxLds);
    ArmDeltaShape preset = a;
    preset.dim = 24; preset.n_layers = 3;  // the presets: inputs and two layers of accumulators, under 40 KB
    CHECK(armdelta_incremental_lds(preset) == 3 * 24 * 512 && ratedelta_path(armdelta_incremental_lds(preset), kArmDeltaAuto) == kArmDeltaIncremental);
    ArmDeltaShape bad = a;
    bad.q_w = -17;  // 16 + q_w < 0: decode_network refuses such a step
    CHECK(armdelta_place(bad, 0, &mv, &index, &shift) == CCD_ERR_VALUE);
    bad = a; bad.q_b = -33;
    CHECK(armdelta_place(bad, armdelta_count(bad) - 1, &mv, &index, &shift) == CCD_ERR_VALUE);
    bad = a; bad.dim = 0;
    CHECK(armdelta_place(bad, 0, &mv, &index, &shift) == CCD_ERR_ARG);
    // the IFCE
    const IfceDeltaShape s = ifcedelta_shape(arch);
    const int64_t n = ifcedelta_count(s);
    CHECK(ifcedelta_place(s, -1, &mv, &index, &shift) == CCD_ERR_ARG && ifcedelta_place(s, n, &mv, &index, &shift) == CCD_ERR_ARG);
    // the scratch lies in the columns of layer 1's and layer 2's accumulators, and the ARM's planning is what it was
    for (int n_hidden = 0; n_hidden <= 7; ++n_hidden) {
        IfceDeltaShape t = s;
        t.arm.dim = 24; t.arm.n_layers = n_hidden + 1;
        CHECK(ifcedelta_incremental_lds(t) == static_cast<int64_t>(1 + n_hidden) * 24 * 512);
        CHECK(armdelta_incremental_lds(t.arm) == static_cast<int64_t>(1 + n_hidden + (n_hidden >= 3 ? 2 : 0)) * 24 * 512);
        CHECK(ifcedelta_incremental_lds(t) >= static_cast<int64_t>(2 + (n_hidden >= 2) + (n_hidden >= 3)) * 24 * 512 || n_hidden == 0);
    }
    IfceDeltaShape iwide = s;
    iwide.arm = wide;
    CHECK(ifcedelta_incremental_lds(iwide) > kArmDeltaMaxLds);
    if (n == 0) return;
    IfceDeltaShape ibad = s;
    ibad.q_w = -17;
    CHECK(ifcedelta_place(ibad, 0, &mv, &index, &shift) == CCD_ERR_VALUE);
    ibad = s; ibad.q_b = -33;
    CHECK(ifcedelta_place(ibad, n - 1, &mv, &index, &shift) == CCD_ERR_VALUE);
    ibad = s; ibad.q_b = 32;  // no 64-bit shift
    CHECK(ifcedelta_place(ibad, n - 1, &mv, &index, &shift) == CCD_ERR_VALUE);
    ibad = s; ibad.n_grids = CCD_MAX_GRIDS + 1;
    CHECK(ifcedelta_place(ibad, 0, &mv, &index, &shift) == CCD_ERR_ARG);
}

struct Counts { long arm = 0, ifce = 0; };
// one network: both tables' plans and the refusals
static Counts check_network(const ccd_cc_header& arch, const std::vector<int32_t>& ints) {
    const Decoded base = decoded(arch, ints);
    Counts c;
    c.arm = check_arm(arch, ints, base);
    c.ifce = check_ifce(arch, ints, base);
    check_refusals(arch);
    return c;
}

// a made-up network: the architecture re-derived from `t`, integers in [-64, 64] from `rng`, and the int32 edges - ints[first]
// at 2^31 - 1 (+1 cannot be transmitted), ints[last] at -2^31 (-1 cannot): both moves are planned as not legal, the other two as legal
static Counts check_made_up(const ccd_cc_header& t, uint64_t& rng, bool ifce_edges) {
    ccd_cc_header arch;
    CHECK(rederive_cc_header(t, 0, &arch) == CCD_OK);
    CHECK(arch.total_context_arm == t.spatial_context_arm + t.output_feature_ifce);
    int64_t n_kind[8], total = 0;
    CHECK(ccd_network_layout(&arch, n_kind) == CCD_OK);
    for (int64_t n : n_kind) total += n;
    auto draw = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    std::vector<int32_t> ints(static_cast<size_t>(total));
    for (int64_t i = 0; i < total; ++i) ints[static_cast<size_t>(i)] = static_cast<int32_t>(draw() % 129) - 64;
    const int64_t n_arm = n_kind[0] + n_kind[1], n_ifce = n_kind[2] + n_kind[3];
    const int64_t first = ifce_edges ? n_arm : 0, last = ifce_edges ? n_arm + n_ifce - 1 : n_arm - 1;
    CHECK(!ifce_edges || n_ifce > 0);
    ints[static_cast<size_t>(first)] = INT32_MAX;
    ints[static_cast<size_t>(last)] = INT32_MIN;
    const Counts c = check_network(arch, ints);
    // all but the two moves that leave int32
    if (ifce_edges) CHECK(c.ifce == 2 * n_ifce - 2);
    else CHECK(n_arm > kWholeTable ? c.arm >= 60 : c.arm == 2 * n_arm - 2);
    RateDeltaMove mv{};
    CHECK(ratedelta_move(1, INT32_MAX, 16, &mv) == CCD_OK && !mv.legal && ratedelta_move(-1, INT32_MAX, 16, &mv) == CCD_OK && mv.legal);
    CHECK(ratedelta_move(-1, INT32_MIN, 32, &mv) == CCD_OK && !mv.legal && ratedelta_move(1, INT32_MIN, 32, &mv) == CCD_OK && mv.legal);
    return c;
}

int main(int argc, char** argv) {
    static ccd_video_header vh;
    int n_cc = 0, n_with = 0;
    Counts total;
    bool have_donor = false;
    ccd_cc_header donor;
    for (int a = 1; a < argc; ++a) {
        const std::vector<uint8_t> bs = read_file(argv[a]);
        int used = read_video_header(bs.data(), bs.size(), &vh);
        CHECK(used > 0);
        size_t pos = static_cast<size_t>(used);
        for (int f = 0; f < vh.n_frames; ++f) {
            ccd_frame_header fh;
            used = read_frame_header(bs.data() + pos, bs.size() - pos, &fh);
            CHECK(used > 0);
            pos += static_cast<size_t>(used);
            for (int c = 0; c < (fh.frame_type == 0 ? 1 : 2); ++c) {
                ccd_cc_header ch;
                used = read_cc_header(bs.data() + pos, bs.size() - pos, &ch);
                CHECK(used > 0);
                pos += static_cast<size_t>(used);
                int64_t n_kind[8], n_ints = 0;
                CHECK(ccd_network_layout(&ch, n_kind) == CCD_OK);
                for (int64_t n : n_kind) n_ints += n;
                std::vector<int32_t> ints(static_cast<size_t>(n_ints));
                CHECK(ccd_network_values(&ch, bs.data() + pos, static_cast<size_t>(ch.nn_n_bytes), ints.data(), n_ints) == n_ints);
                const Counts got = check_network(ch, ints);
                CHECK((got.ifce > 0) == (n_kind[2] + n_kind[3] > 0));
                total.arm += got.arm;
                total.ifce += got.ifce;
                n_with += got.ifce > 0 ? 1 : 0;
                if (!have_donor) { donor = ch; have_donor = true; }
                ++n_cc;
                pos += static_cast<size_t>(ch.nn_n_bytes) + static_cast<size_t>(ch.n_bytes_latent);
            }
        }
        CHECK(pos == bs.size());
    }
    CHECK(have_donor);
    // tests/arm_layouts.py: (spatial contexts, IFCE features, hidden layers) at the donor's size
    static const int kArmShapes[][3] = {{40, 31, 7}, {40, 25, 1}, {39, 31, 0}, {40, 24, 2}, {1, 0, 0}, {1, 31, 7}, {3, 2, 4}, {2, 7, 5},
                                        {6, 3, 3}, {9, 7, 6}, {5, 2, 1}, {6, 0, 2}};
    int n_arm_shapes = 0, n_ifce_shapes = 0;
    uint64_t rng = 0x9e3779b97f4a7c15ull;
    for (const auto& sh : kArmShapes) {
        ccd_cc_header t = donor;
        t.spatial_context_arm = sh[0]; t.output_feature_ifce = sh[1]; t.n_hidden_layers_arm = sh[2];
        if (sh[1] == 0) t.has_ifce_resolution = 0;
        total.arm += check_made_up(t, rng, false).arm;
        ++n_arm_shapes;
    }
    // tests/arm_layouts.py: (spatial contexts, IFCE features, hidden layers, ifce_resolution) of its cases with IFCE, at 18 x 65
    static const int kIfceShapes[][5] = {{6, 3, 3, 0, 15}, {9, 7, 6, 0, 15}, {6, 3, 3, 3, 15}, {9, 7, 6, 3, 15}, {6, 3, 3, 1, 1}, {9, 7, 6, 1, 1},
                                         {6, 3, 3, 4, 4},  {9, 7, 6, 4, 4},  {5, 2, 1, 0, 15}, {40, 31, 7, 0, 2}, {40, 25, 1, 0, 2}, {39, 31, 0, 0, 2},
                                         {40, 24, 2, 0, 2}, {1, 31, 7, 0, 2}, {3, 2, 4, 0, 2},  {2, 7, 5, 0, 2}};
    bool saw_gap = false, saw_last = false, saw_two = false;  // a grid without IFCE above one with; IFCE on the last grid; fin >= 2
    rng = 0x9e3779b97f4a7c15ull;
    for (const auto& sh : kIfceShapes) {
        ccd_cc_header t = donor, arch;
        t.spatial_context_arm = sh[0]; t.output_feature_ifce = sh[1]; t.n_hidden_layers_arm = sh[2];
        t.has_ifce_resolution = 1; t.ifce_resolution[0] = sh[3]; t.ifce_resolution[1] = sh[4];
        t.img_size[0] = 18; t.img_size[1] = 65;
        CHECK(rederive_cc_header(t, 0, &arch) == CCD_OK);
        for (int g = 0; g < arch.n_grids; ++g) {
            saw_gap |= g + 1 < arch.n_grids && arch.input_features_ifce[g] == 0 && arch.input_features_ifce[g + 1] > 0;
            saw_two |= arch.input_features_ifce[g] >= 2;
        }
        saw_last |= arch.input_features_ifce[arch.n_grids - 1] > 0;
        total.ifce += check_made_up(t, rng, true).ifce;
        ++n_ifce_shapes;
    }
    CHECK(saw_gap && saw_last && saw_two);
    std::printf("ratedelta_host_check: %d cool-chics of %d streams (%d with IFCE); ARM: %d made-up shapes, %ld candidates; "
                "IFCE: %d made-up shapes, %ld candidates: ok\n", n_cc, argc - 1, n_with, n_arm_shapes, total.arm, n_ifce_shapes, total.ifce);
    return 0;
}
