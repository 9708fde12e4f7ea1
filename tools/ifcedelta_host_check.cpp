// ifcedelta_host_check.cpp - the planning of the IFCE parameter table (cool_chic_amd/csrc/ccd_ifcedelta_plan.hpp, DESIGN.md
// section 4.21) against decode_network, as a stand-alone CPU program: meant to be built with -fsanitize=address,undefined together
// with the two host sources it exercises, host code only (no device code is compiled, no device is needed, and the sanitizers
// are never asked of an offload target):
//
//   hipcc --offload-host-only -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/ifcedelta_host_check.cpp cool_chic_amd/csrc/ccd_format.cpp cool_chic_amd/csrc/ccd_writer.cpp -o ifcedelta_host_check
//   ./ifcedelta_host_check tests/golden/*.cool
//
// Every cool-chic of every stream that has IFCE integers, and the IFCE cases of tests/arm_layouts.py (its placements and its
// shapes with IFCE features, at 18 x 65) made from the first cool-chic's architecture with seeded integers: the plan of every
// (k, s) is checked (range, no entry shared by two parameters, every IFCE entry some parameter's), then values[k] + s is
// encoded again (ccd_encode_network), decoded (decode_network), and ALL fixed-point IFCE blocks and the whole fixed-point ARM
// are compared with the plan: exactly the planned entry differs, by exactly the planned increment, and the ARM not at all.
// Then the int32 edges (the first weight at 2^31 - 1, the last bias at -2^31) and the refusals.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../cool_chic_amd/csrc/ccd_format.hpp"
#include "../cool_chic_amd/csrc/ccd_ifcedelta_plan.hpp"

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

// the fixed-point networks in the order the kernels read them (pack_int_networks): the ARM, and per grid the IFCE block
struct Decoded {
    std::vector<int64_t> arm;
    std::vector<std::vector<int64_t>> ifce;  // [n_grids]: w[fin][n_if], b[n_if]; empty without IFCE
};
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
    Decoded d;
    for (const FixedLayer& L : net.arm.layers) { d.arm.insert(d.arm.end(), L.w.begin(), L.w.end()); d.arm.insert(d.arm.end(), L.b.begin(), L.b.end()); }
    d.arm.insert(d.arm.end(), net.arm.ws.begin(), net.arm.ws.end());
    d.arm.insert(d.arm.end(), net.arm.bs.begin(), net.arm.bs.end());
    d.ifce.resize(static_cast<size_t>(h.n_grids));
    for (int g = 0; g < h.n_grids; ++g) {
        if (net.ifce[static_cast<size_t>(g)].dim == 0) continue;
        const FixedLayer& L = net.ifce[static_cast<size_t>(g)].layers[0];
        d.ifce[static_cast<size_t>(g)].insert(d.ifce[static_cast<size_t>(g)].end(), L.w.begin(), L.w.end());
        d.ifce[static_cast<size_t>(g)].insert(d.ifce[static_cast<size_t>(g)].end(), L.b.begin(), L.b.end());
    }
    return d;
}

// every (k, s) of one network; returns the number of candidates decoded
static long check_network(const ccd_cc_header& arch, std::vector<int32_t> ints) {
    const IfceDeltaShape shape = ifcedelta_shape(arch);
    int64_t n_kind[8];
    CHECK(ccd_network_layout(&arch, n_kind) == CCD_OK);
    const int64_t n_arm = n_kind[0] + n_kind[1], n_ifce = n_kind[2] + n_kind[3];
    CHECK(ifcedelta_count(shape) == n_ifce && ifcedelta_n_weights(shape) == n_kind[2] && ifcedelta_n_biases(shape) == n_kind[3]);
    if (n_ifce == 0) return 0;
    const Decoded base = decoded(arch, ints);
    const int n_if = shape.n_ifce_out;
    std::vector<std::vector<char>> seen(base.ifce.size());
    for (int g = 0; g < shape.n_grids; ++g) {
        CHECK(static_cast<int64_t>(base.ifce[static_cast<size_t>(g)].size()) == (shape.fin[g] > 0 ? static_cast<int64_t>(shape.fin[g] + 1) * n_if : 0));
        seen[static_cast<size_t>(g)].assign(base.ifce[static_cast<size_t>(g)].size(), 0);
    }
    long n = 0;
    int last_grid_w = 0, last_grid_b = 0;
    for (int64_t k = 0; k < n_ifce; ++k)
        for (int sign = -1; sign <= 1; sign += 2) {
            IfceDeltaMove mv{};
            int64_t index = -1;
            const size_t at = static_cast<size_t>(n_arm + k);
            CHECK(ifcedelta_move(shape, k, sign, ints[at], &mv, &index) == CCD_OK);
            CHECK(mv.grid >= 0 && mv.grid < shape.n_grids && shape.fin[mv.grid] > 0 && mv.out >= 0 && mv.out < n_if && mv.in >= -1 &&
                  mv.in < shape.fin[mv.grid]);
            CHECK(index >= 0 && index < static_cast<int64_t>(base.ifce[static_cast<size_t>(mv.grid)].size()));
            CHECK((mv.in < 0) == (k >= n_kind[2]));
            // stream order: the grids ascend inside the weights and inside the biases
            int& last = mv.in < 0 ? last_grid_b : last_grid_w;
            CHECK(mv.grid >= last);
            last = mv.grid;
            const int64_t moved = static_cast<int64_t>(ints[at]) + sign;
            CHECK(mv.legal == (moved >= INT32_MIN && moved <= INT32_MAX));
            char& mark = seen[static_cast<size_t>(mv.grid)][static_cast<size_t>(index)];
            if (sign < 0) { CHECK(!mark); mark = 1; }  // no two parameters share an entry
            if (!mv.legal) continue;
            const int32_t keep = ints[at];
            ints[at] = static_cast<int32_t>(moved);
            const Decoded got = decoded(arch, ints);
            ints[at] = keep;
            CHECK(got.arm == base.arm);  // the ARM does not differ at all
            CHECK(got.ifce.size() == base.ifce.size());
            for (size_t g = 0; g < base.ifce.size(); ++g) {
                CHECK(got.ifce[g].size() == base.ifce[g].size());
                for (size_t i = 0; i < base.ifce[g].size(); ++i) {
                    const bool planned = static_cast<int>(g) == mv.grid && static_cast<int64_t>(i) == index;
                    CHECK(static_cast<uint64_t>(got.ifce[g][i]) == static_cast<uint64_t>(base.ifce[g][i]) + (planned ? static_cast<uint64_t>(mv.inc) : 0));
                }
            }
            ++n;
        }
    for (const auto& grid : seen) for (char s : grid) CHECK(s);  // every IFCE entry is some parameter's
    return n;
}

static void check_refusals(const ccd_cc_header& arch) {
    IfceDeltaShape s = ifcedelta_shape(arch);
    IfceDeltaMove mv{};
    int64_t index = 0;
    int shift = 0;
    const int64_t n = ifcedelta_count(s);
    CHECK(ifcedelta_place(s, -1, &mv, &index, &shift) == CCD_ERR_ARG && ifcedelta_place(s, n, &mv, &index, &shift) == CCD_ERR_ARG);
    CHECK(ifcedelta_path(s, -1) == CCD_ERR_ARG && ifcedelta_path(s, 3) == CCD_ERR_ARG);
    CHECK(ifcedelta_path(s, kArmDeltaGeneric) == kArmDeltaGeneric);
    const bool fits = ifcedelta_incremental_lds(s) <= kArmDeltaMaxLds;
    CHECK(ifcedelta_path(s, kArmDeltaAuto) == (fits ? kArmDeltaIncremental : kArmDeltaGeneric));
    CHECK(ifcedelta_path(s, kArmDeltaIncremental) == (fits ? kArmDeltaIncremental : CCD_ERR_UNSUPPORTED));
    // the scratch lies in the columns of layer 1's and layer 2's accumulators, and the ARM's planning is what it was
    for (int n_hidden = 0; n_hidden <= 7; ++n_hidden) {
        IfceDeltaShape t = s;
        t.arm.dim = 24; t.arm.n_layers = n_hidden + 1;
        CHECK(ifcedelta_incremental_lds(t) == static_cast<int64_t>(1 + n_hidden) * 24 * 512);
        CHECK(armdelta_incremental_lds(t.arm) == static_cast<int64_t>(1 + n_hidden + (n_hidden >= 3 ? 2 : 0)) * 24 * 512);
        CHECK(ifcedelta_incremental_lds(t) >= static_cast<int64_t>(2 + (n_hidden >= 2) + (n_hidden >= 3)) * 24 * 512 || n_hidden == 0);
    }
    IfceDeltaShape wide = s;
    wide.arm.dim = 71; wide.arm.n_layers = 8;  // 10 x 71 columns of per-lane state: beyond the LDS
    CHECK(ifcedelta_incremental_lds(wide) > kArmDeltaMaxLds && ifcedelta_path(wide, kArmDeltaIncremental) == CCD_ERR_UNSUPPORTED &&
          ifcedelta_path(wide, kArmDeltaAuto) == kArmDeltaGeneric);
    if (n == 0) return;
    CHECK(ifcedelta_move(s, 0, 0, 0, &mv, &index) == CCD_ERR_ARG && ifcedelta_move(s, 0, 2, 0, &mv, &index) == CCD_ERR_ARG);
    IfceDeltaShape bad = s;
    bad.q_w = -17;  // 16 + q_w < 0: decode_network refuses such a step
    CHECK(ifcedelta_place(bad, 0, &mv, &index, &shift) == CCD_ERR_VALUE);
    bad = s; bad.q_b = -33;
    CHECK(ifcedelta_place(bad, n - 1, &mv, &index, &shift) == CCD_ERR_VALUE);
    bad = s; bad.q_b = 32;  // no 64-bit shift
    CHECK(ifcedelta_place(bad, n - 1, &mv, &index, &shift) == CCD_ERR_VALUE);
    bad = s; bad.n_grids = CCD_MAX_GRIDS + 1;
    CHECK(ifcedelta_place(bad, 0, &mv, &index, &shift) == CCD_ERR_ARG);
}

int main(int argc, char** argv) {
    static ccd_video_header vh;
    int n_cc = 0, n_with = 0, n_shapes = 0;
    long n_cand = 0;
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
                int64_t n_kind[8], total = 0;
                CHECK(ccd_network_layout(&ch, n_kind) == CCD_OK);
                for (int64_t n : n_kind) total += n;
                std::vector<int32_t> ints(static_cast<size_t>(total));
                CHECK(ccd_network_values(&ch, bs.data() + pos, static_cast<size_t>(ch.nn_n_bytes), ints.data(), total) == total);
                const long got = check_network(ch, ints);
                CHECK((got > 0) == (n_kind[2] + n_kind[3] > 0));
                n_cand += got;
                n_with += got > 0 ? 1 : 0;
                check_refusals(ch);
                if (!have_donor) { donor = ch; have_donor = true; }
                ++n_cc;
                pos += static_cast<size_t>(ch.nn_n_bytes) + static_cast<size_t>(ch.n_bytes_latent);
            }
        }
        CHECK(pos == bs.size());
    }
    CHECK(have_donor);
    // tests/arm_layouts.py: (spatial contexts, IFCE features, hidden layers, ifce_resolution) of its cases with IFCE
    static const int kShapes[][5] = {{6, 3, 3, 0, 15}, {9, 7, 6, 0, 15}, {6, 3, 3, 3, 15}, {9, 7, 6, 3, 15}, {6, 3, 3, 1, 1}, {9, 7, 6, 1, 1},
                                     {6, 3, 3, 4, 4},  {9, 7, 6, 4, 4},  {5, 2, 1, 0, 15}, {40, 31, 7, 0, 2}, {40, 25, 1, 0, 2}, {39, 31, 0, 0, 2},
                                     {40, 24, 2, 0, 2}, {1, 31, 7, 0, 2}, {3, 2, 4, 0, 2},  {2, 7, 5, 0, 2}};
    uint64_t rng = 0x9e3779b97f4a7c15ull;
    auto draw = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    bool saw_gap = false, saw_last = false, saw_two = false;  // a grid without IFCE above one with; IFCE on the last grid; fin >= 2
    for (const auto& sh : kShapes) {
        ccd_cc_header t = donor, arch;
        t.spatial_context_arm = sh[0]; t.output_feature_ifce = sh[1]; t.n_hidden_layers_arm = sh[2];
        t.has_ifce_resolution = 1; t.ifce_resolution[0] = sh[3]; t.ifce_resolution[1] = sh[4];
        t.img_size[0] = 18; t.img_size[1] = 65;
        CHECK(rederive_cc_header(t, 0, &arch) == CCD_OK);
        CHECK(arch.total_context_arm == sh[0] + sh[1]);
        int64_t n_kind[8], total = 0;
        CHECK(ccd_network_layout(&arch, n_kind) == CCD_OK);
        for (int64_t n : n_kind) total += n;
        const int64_t n_arm = n_kind[0] + n_kind[1], n_ifce = n_kind[2] + n_kind[3];
        CHECK(n_ifce > 0);
        for (int g = 0; g < arch.n_grids; ++g) {
            saw_gap |= g + 1 < arch.n_grids && arch.input_features_ifce[g] == 0 && arch.input_features_ifce[g + 1] > 0;
            saw_two |= arch.input_features_ifce[g] >= 2;
        }
        saw_last |= arch.input_features_ifce[arch.n_grids - 1] > 0;
        std::vector<int32_t> ints(static_cast<size_t>(total));
        for (int64_t i = 0; i < total; ++i) ints[static_cast<size_t>(i)] = static_cast<int32_t>(draw() % 129) - 64;
        // the int32 edges: the first IFCE weight at 2^31 - 1 (+1 cannot be transmitted), the last IFCE bias at -2^31 (-1 cannot)
        ints[static_cast<size_t>(n_arm)] = INT32_MAX;
        ints[static_cast<size_t>(n_arm + n_ifce - 1)] = INT32_MIN;
        const long got = check_network(arch, ints);
        CHECK(got == 2 * n_ifce - 2);  // all but the two moves that leave int32
        n_cand += got;
        IfceDeltaMove mv{};
        int64_t index = 0;
        const IfceDeltaShape shape = ifcedelta_shape(arch);
        CHECK(ifcedelta_move(shape, 0, 1, INT32_MAX, &mv, &index) == CCD_OK && !mv.legal);
        CHECK(ifcedelta_move(shape, 0, -1, INT32_MAX, &mv, &index) == CCD_OK && mv.legal);
        CHECK(ifcedelta_move(shape, n_ifce - 1, -1, INT32_MIN, &mv, &index) == CCD_OK && !mv.legal);
        CHECK(ifcedelta_move(shape, n_ifce - 1, 1, INT32_MIN, &mv, &index) == CCD_OK && mv.legal);
        check_refusals(arch);
        ++n_shapes;
    }
    CHECK(saw_gap && saw_last && saw_two);
    std::printf("ifcedelta_host_check: %d cool-chics of %d streams (%d with IFCE) and %d made-up IFCE shapes, %ld candidates: ok\n", n_cc,
                argc - 1, n_with, n_shapes, n_cand);
    return 0;
}
