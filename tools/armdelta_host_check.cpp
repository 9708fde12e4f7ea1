// armdelta_host_check.cpp - the planning of the ARM parameter table (cool_chic_amd/csrc/ccd_armdelta_plan.hpp, DESIGN.md section
// 4.20) against decode_network, as a stand-alone CPU program: meant to be built with -fsanitize=address,undefined together with
// the two host sources it exercises, host code only (no device code is compiled, no device is needed, and the sanitizers are
// never asked of an offload target):
//
//   hipcc --offload-host-only -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/armdelta_host_check.cpp cool_chic_amd/csrc/ccd_format.cpp cool_chic_amd/csrc/ccd_writer.cpp -o armdelta_host_check
//   ./armdelta_host_check tests/golden/*.cool
//
// Every cool-chic of every stream, and the ARM shapes of tests/arm_layouts.py (ARM_SHAPES, PLACEMENT_SHAPES, TINY_SHAPES) made
// from the first cool-chic's architecture with seeded integers: for every ARM integer k and both signs, values[k] + s is encoded
// again (ccd_encode_network), decoded (decode_network), and the fixed-point ARM must differ from the base's in exactly the planned
// entry by exactly the planned increment.  Networks of more than 2 048 ARM integers have the plan of every (k, s) checked (range,
// no entry shared, every entry covered) and the decode within 8 parameters of every layer's first weight, of the first bias and
// of both ends: the whole program then takes about two minutes under the sanitizers.  Then the int32 edges (a weight at 2^31 - 1, a bias at -2^31) and the refusals.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../cool_chic_amd/csrc/ccd_armdelta_plan.hpp"
#include "../cool_chic_amd/csrc/ccd_format.hpp"

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

// the fixed-point ARM in the order the kernels read it (pack_int_networks)
static std::vector<int64_t> flat_arm(const FixedArm& a) {
    std::vector<int64_t> out;
    for (const FixedLayer& L : a.layers) { out.insert(out.end(), L.w.begin(), L.w.end()); out.insert(out.end(), L.b.begin(), L.b.end()); }
    out.insert(out.end(), a.ws.begin(), a.ws.end());
    out.insert(out.end(), a.bs.begin(), a.bs.end());
    return out;
}

static std::vector<int64_t> decoded_arm(const ccd_cc_header& arch, const std::vector<int32_t>& ints) {
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
    return flat_arm(net.arm);
}

constexpr int64_t kWholeTable = 2048;
// first weight of layer l in STREAM order (l == n_layers: the stabiliser's)
static int64_t armdelta_layer_weights_first(const ArmDeltaShape& s, int l) {
    return l < s.n_layers ? static_cast<int64_t>(l) * s.dim * s.dim : static_cast<int64_t>(s.n_layers - 1) * s.dim * s.dim + 2 * s.dim;
}
// every (k, s) of one network; returns the number of candidates decoded
static long check_network(const ccd_cc_header& arch, std::vector<int32_t> ints) {
    const ArmDeltaShape shape = armdelta_shape(arch);
    int64_t n_kind[8];
    CHECK(ccd_network_layout(&arch, n_kind) == CCD_OK);
    const int64_t n_arm = n_kind[0] + n_kind[1];
    CHECK(armdelta_count(shape) == n_arm && armdelta_n_weights(shape) == n_kind[0] && armdelta_n_biases(shape) == n_kind[1]);
    const std::vector<int64_t> base = decoded_arm(arch, ints);
    CHECK(static_cast<int64_t>(base.size()) == armdelta_layer_first(shape, shape.n_layers) + 2 * shape.dim + 2);
    std::vector<char> seen(base.size(), 0);
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
            ArmDeltaMove mv{};
            int64_t index = -1;
            CHECK(armdelta_move(shape, k, sign, ints[static_cast<size_t>(k)], &mv, &index) == CCD_OK);
            CHECK(index >= 0 && index < static_cast<int64_t>(base.size()));
            CHECK(mv.layer >= 0 && mv.layer <= shape.n_layers && mv.out >= 0 && mv.out < (mv.layer < shape.n_layers - 1 ? shape.dim : 2) &&
                  mv.in >= -1 && mv.in < shape.dim);
            CHECK(shape.stabiliser || mv.layer < shape.n_layers);
            const int64_t moved = static_cast<int64_t>(ints[static_cast<size_t>(k)]) + sign;
            CHECK(mv.legal == (moved >= INT32_MIN && moved <= INT32_MAX));
            if (sign < 0) { CHECK(!seen[static_cast<size_t>(index)]); seen[static_cast<size_t>(index)] = 1; }  // no two parameters share an entry
            if (!mv.legal) continue;
            if (n_arm > kWholeTable && !near_mark(k)) continue;
            const int32_t keep = ints[static_cast<size_t>(k)];
            ints[static_cast<size_t>(k)] = static_cast<int32_t>(moved);
            const std::vector<int64_t> got = decoded_arm(arch, ints);
            ints[static_cast<size_t>(k)] = keep;
            CHECK(got.size() == base.size());
            for (size_t i = 0; i < base.size(); ++i) {
                const uint64_t want = static_cast<uint64_t>(base[i]) + (static_cast<int64_t>(i) == index ? static_cast<uint64_t>(mv.inc) : 0);
                CHECK(static_cast<uint64_t>(got[i]) == want);
            }
            ++n;
        }
    if (shape.stabiliser) for (char s : seen) CHECK(s);  // every entry of the fixed-point ARM is some parameter's
    return n;
}

static void check_refusals(const ccd_cc_header& arch) {
    ArmDeltaShape s = armdelta_shape(arch);
    ArmDeltaMove mv{};
    int64_t index = 0;
    int shift = 0;
    CHECK(armdelta_place(s, -1, &mv, &index, &shift) == CCD_ERR_ARG && armdelta_place(s, armdelta_count(s), &mv, &index, &shift) == CCD_ERR_ARG);
    CHECK(armdelta_move(s, 0, 0, 0, &mv, &index) == CCD_ERR_ARG && armdelta_move(s, 0, 2, 0, &mv, &index) == CCD_ERR_ARG);
    CHECK(armdelta_path(s, -1) == CCD_ERR_ARG && armdelta_path(s, 3) == CCD_ERR_ARG);
    CHECK(armdelta_path(s, kArmDeltaGeneric) == kArmDeltaGeneric);
    const bool fits = armdelta_incremental_lds(s) <= kArmDeltaMaxLds;
    CHECK(armdelta_path(s, kArmDeltaAuto) == (fits ? kArmDeltaIncremental : kArmDeltaGeneric));
    CHECK(armdelta_path(s, kArmDeltaIncremental) == (fits ? kArmDeltaIncremental : CCD_ERR_UNSUPPORTED));
    ArmDeltaShape wide = s;
    wide.dim = 71; wide.n_layers = 8;  // 10 x 71 columns of per-lane state: beyond the LDS
    CHECK(armdelta_incremental_lds(wide) > kArmDeltaMaxLds && armdelta_path(wide, kArmDeltaIncremental) == CCD_ERR_UNSUPPORTED &&
          armdelta_path(wide, kArmDeltaAuto) == kArmDeltaGeneric);
    ArmDeltaShape preset = s;
    preset.dim = 24; preset.n_layers = 3;  // the presets: inputs and two layers of accumulators, under 40 KB
    CHECK(armdelta_incremental_lds(preset) == 3 * 24 * 512 && armdelta_path(preset, kArmDeltaAuto) == kArmDeltaIncremental);
    ArmDeltaShape bad = s;
    bad.q_w = -17;  // 16 + q_w < 0: decode_network refuses such a step
    CHECK(armdelta_place(bad, 0, &mv, &index, &shift) == CCD_ERR_VALUE);
    bad = s; bad.q_b = -33;
    CHECK(armdelta_place(bad, armdelta_count(bad) - 1, &mv, &index, &shift) == CCD_ERR_VALUE);
    bad = s; bad.dim = 0;
    CHECK(armdelta_place(bad, 0, &mv, &index, &shift) == CCD_ERR_ARG);
}

int main(int argc, char** argv) {
    static ccd_video_header vh;
    int n_cc = 0, n_shapes = 0;
    long n_cand = 0;
    bool have_donor = false;
    ccd_cc_header donor;
    std::vector<int32_t> donor_ints;
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
                n_cand += check_network(ch, ints);
                check_refusals(ch);
                if (!have_donor) { donor = ch; donor_ints = ints; have_donor = true; }
                ++n_cc;
                pos += static_cast<size_t>(ch.nn_n_bytes) + static_cast<size_t>(ch.n_bytes_latent);
            }
        }
        CHECK(pos == bs.size());
    }
    CHECK(have_donor);
    // tests/arm_layouts.py: (spatial contexts, IFCE features, hidden layers)
    static const int kShapes[][3] = {{40, 31, 7}, {40, 25, 1}, {39, 31, 0}, {40, 24, 2}, {1, 0, 0}, {1, 31, 7}, {3, 2, 4}, {2, 7, 5},
                                     {6, 3, 3}, {9, 7, 6}, {5, 2, 1}, {6, 0, 2}};
    uint64_t rng = 0x9e3779b97f4a7c15ull;
    auto draw = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    for (const auto& sh : kShapes) {
        ccd_cc_header t = donor, arch;
        t.spatial_context_arm = sh[0]; t.output_feature_ifce = sh[1]; t.n_hidden_layers_arm = sh[2];
        if (sh[1] == 0) t.has_ifce_resolution = 0;
        CHECK(rederive_cc_header(t, 0, &arch) == CCD_OK);
        CHECK(arch.total_context_arm == sh[0] + sh[1]);
        int64_t n_kind[8], total = 0;
        CHECK(ccd_network_layout(&arch, n_kind) == CCD_OK);
        for (int64_t n : n_kind) total += n;
        std::vector<int32_t> ints(static_cast<size_t>(total));
        for (int64_t i = 0; i < total; ++i) ints[static_cast<size_t>(i)] = static_cast<int32_t>(draw() % 129) - 64;
        const int64_t n_arm = n_kind[0] + n_kind[1];
        // the int32 edges: the first weight at 2^31 - 1 (+1 cannot be transmitted), the last bias at -2^31 (-1 cannot)
        ints[0] = INT32_MAX;
        ints[static_cast<size_t>(n_arm - 1)] = INT32_MIN;
        const long before = n_cand;
        n_cand += check_network(arch, ints);
        CHECK(n_arm > kWholeTable ? n_cand - before >= 60 : n_cand - before == 2 * n_arm - 2);  // all but the two moves that leave int32
        ArmDeltaMove mv{};
        int64_t index = 0;
        const ArmDeltaShape shape = armdelta_shape(arch);
        CHECK(armdelta_move(shape, 0, 1, ints[0], &mv, &index) == CCD_OK && !mv.legal);
        CHECK(armdelta_move(shape, 0, -1, ints[0], &mv, &index) == CCD_OK && mv.legal);
        CHECK(armdelta_move(shape, n_arm - 1, -1, ints[static_cast<size_t>(n_arm - 1)], &mv, &index) == CCD_OK && !mv.legal);
        CHECK(armdelta_move(shape, n_arm - 1, 1, ints[static_cast<size_t>(n_arm - 1)], &mv, &index) == CCD_OK && mv.legal);
        check_refusals(arch);
        ++n_shapes;
    }
    std::printf("armdelta_host_check: %d cool-chics of %d streams and %d made-up ARM shapes, %ld candidates: ok\n", n_cc, argc - 1, n_shapes, n_cand);
    return 0;
}
