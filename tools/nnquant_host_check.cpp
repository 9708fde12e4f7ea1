// nnquant_host_check.cpp - the host primitives of the network quantisation search over real streams
// and over the refusal cases, as a stand-alone CPU program: meant to be built with -fsanitize=address,undefined together with
// the two host sources it exercises, host code only (no device code is compiled, no device is needed, and the sanitizers are
// never asked of an offload target):
//
//   hipcc --offload-host-only -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/nnquant_host_check.cpp cool_chic_amd/csrc/ccd_format.cpp cool_chic_amd/csrc/ccd_writer.cpp -o nnquant_host_check
//   ./nnquant_host_check tests/golden/*.cool
//
// Every cool-chic of every stream: ccd_network_values, re-encoded byte for byte; quantise(dequantise) at every step of every
// group; the best Exp-Golomb orders, whose payload has ceil(sum of bits / 8) bytes and decodes to the same integers.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../cool_chic_amd/csrc/ccd_format.hpp"  // the header parsers without the device runtime (ccd_read_* live beside it)

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

static const int kCount[8] = {9, 17, 9, 17, 13, 1, 13, 25}, kFirst[8] = {-8, -16, -8, -16, -12, 0, -12, -24};

static std::vector<uint8_t> read_file(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    CHECK(f);
    std::vector<uint8_t> out;
    uint8_t buf[65536];
    for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;) out.insert(out.end(), buf, buf + n);
    std::fclose(f);
    return out;
}

static int check_coolchic(const ccd_cc_header& arch, const uint8_t* nn, size_t n_nn) {
    int64_t n_kind[8], total = 0;
    CHECK(ccd_network_layout(&arch, n_kind) == CCD_OK);
    for (int64_t n : n_kind) total += n;
    std::vector<int32_t> ints(static_cast<size_t>(total) + 1, 0x5a5a5a5a);
    CHECK(ccd_network_values(&arch, nn, n_nn, ints.data(), total - 1) == CCD_ERR_ARG);
    CHECK(ccd_network_values(&arch, nn, n_nn, ints.data(), total) == total);
    CHECK(ints[static_cast<size_t>(total)] == 0x5a5a5a5a);
    ints.resize(static_cast<size_t>(total));
    {   // the payload again, with the stream's own orders
        ccd_cc_header h = arch;
        int32_t pad = -1;
        uint8_t* out = nullptr;
        const int64_t n = ccd_encode_network(&h, ints.data(), total, &pad, &out);
        CHECK(n == static_cast<int64_t>(n_nn) && pad == arch.nn_n_bit_pad && std::memcmp(out, nn, n_nn) == 0);
        std::free(out);  // (ccd_free, which lives with the device runtime)
    }
    std::vector<float> x(ints.size());
    std::vector<int32_t> back(ints.size());
    int32_t steps[8];
    for (int g = 0; g < 8; ++g)
        for (int q = kFirst[g]; q < kFirst[g] + kCount[g]; ++q) {
            std::memcpy(steps, arch.nn_q_step_log2, sizeof(steps));
            steps[g] = q;
            size_t at = 0;
            for (int k = 0; k < 8; ++k)
                for (int64_t i = 0; i < n_kind[k]; ++i, ++at) x[at] = std::ldexp(static_cast<float>(ints[at]), steps[k]);
            CHECK(ccd_quantise_network(&arch, x.data(), total, steps, back.data()) == CCD_OK);
            CHECK(back == ints);
        }
    int32_t order[8];
    int64_t bits[8], sum = 0;
    CHECK(ccd_network_best_expgol(&arch, ints.data(), total, order, bits) == CCD_OK);
    ccd_cc_header h = arch;
    for (int g = 0; g < 8; ++g) { CHECK(order[g] >= 0 && order[g] <= 12 && (n_kind[g] > 0 || (order[g] == 0 && bits[g] == 0))); h.nn_expgol_cnt[g] = order[g]; sum += bits[g]; }
    int32_t pad = -1;
    uint8_t* out = nullptr;
    const int64_t n = ccd_encode_network(&h, ints.data(), total, &pad, &out);
    CHECK(n == (sum + 7) / 8 && pad == 8 * n - sum);
    h.nn_n_bit_pad = pad;
    CHECK(ccd_network_values(&h, out, static_cast<size_t>(n), back.data(), total) == total && back == ints);
    std::free(out);  // (ccd_free, which lives with the device runtime)
    // refusals
    std::memcpy(steps, arch.nn_q_step_log2, sizeof(steps));
    for (int g = 0; g < 8; ++g)
        for (int bad : {kFirst[g] - 1, kFirst[g] + kCount[g]}) {
            int32_t s[8];
            std::memcpy(s, steps, sizeof(s));
            s[g] = bad;
            CHECK(ccd_quantise_network(&arch, x.data(), total, s, back.data()) == CCD_ERR_VALUE);
        }
    for (float bad : {std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN(),
                      std::ldexp(1.0f, 31 + steps[0]), std::ldexp(-1.0f, 32 + steps[0]), std::numeric_limits<float>::max()}) {
        std::vector<float> y(x);
        y[0] = bad;
        CHECK(ccd_quantise_network(&arch, y.data(), total, steps, back.data()) == CCD_ERR_VALUE);
    }
    {
        std::vector<float> y(x);
        y[0] = std::ldexp(-1.0f, 31 + steps[0]);  // -2^31 itself is a value
        CHECK(ccd_quantise_network(&arch, y.data(), total, steps, back.data()) == CCD_OK && back[0] == std::numeric_limits<int32_t>::min());
        CHECK(ccd_network_best_expgol(&arch, back.data(), total, order, bits) == CCD_OK);
    }
    CHECK(ccd_quantise_network(&arch, x.data(), total - 1, steps, back.data()) == CCD_ERR_ARG);
    CHECK(ccd_network_best_expgol(&arch, ints.data(), total + 1, order, bits) == CCD_ERR_ARG);
    CHECK(ccd_network_values(&arch, nn, n_nn > 2 ? n_nn - 2 : 0, back.data(), total) < 0 || total == 0);  // a truncated payload
    CHECK(ccd_network_values(nullptr, nn, n_nn, back.data(), total) == CCD_ERR_ARG && ccd_network_values(&arch, nullptr, 0, back.data(), total) == CCD_ERR_ARG &&
          ccd_network_values(&arch, nn, n_nn, nullptr, total) == CCD_ERR_ARG);
    CHECK(ccd_quantise_network(nullptr, x.data(), total, steps, back.data()) == CCD_ERR_ARG && ccd_quantise_network(&arch, nullptr, total, steps, back.data()) == CCD_ERR_ARG &&
          ccd_quantise_network(&arch, x.data(), total, nullptr, back.data()) == CCD_ERR_ARG && ccd_quantise_network(&arch, x.data(), total, steps, nullptr) == CCD_ERR_ARG);
    CHECK(ccd_network_best_expgol(nullptr, ints.data(), total, order, bits) == CCD_ERR_ARG && ccd_network_best_expgol(&arch, nullptr, total, order, bits) == CCD_ERR_ARG &&
          ccd_network_best_expgol(&arch, ints.data(), total, nullptr, bits) == CCD_ERR_ARG && ccd_network_best_expgol(&arch, ints.data(), total, order, nullptr) == CCD_ERR_ARG);
    return static_cast<int>(total);
}

int main(int argc, char** argv) {
    static ccd_video_header vh;
    for (int g = 0; g < 8; ++g) {
        int32_t first = 99;
        CHECK(ccd_q_step_table(g, &first) == kCount[g] && first == kFirst[g]);
    }
    {
        int32_t first = 99;
        CHECK(ccd_q_step_table(-1, &first) == CCD_ERR_ARG && ccd_q_step_table(8, &first) == CCD_ERR_ARG && ccd_q_step_table(0, nullptr) == CCD_ERR_ARG && first == 99);
    }
    int n_cc = 0;
    long n_values = 0;
    for (int a = 1; a < argc; ++a) {
        const std::vector<uint8_t> bs = read_file(argv[a]);
        int used = ccd::read_video_header(bs.data(), bs.size(), &vh);
        CHECK(used > 0);
        size_t pos = static_cast<size_t>(used);
        for (int f = 0; f < vh.n_frames; ++f) {
            ccd_frame_header fh;
            used = ccd::read_frame_header(bs.data() + pos, bs.size() - pos, &fh);
            CHECK(used > 0);
            pos += static_cast<size_t>(used);
            for (int c = 0; c < (fh.frame_type == 0 ? 1 : 2); ++c) {
                ccd_cc_header ch;
                used = ccd::read_cc_header(bs.data() + pos, bs.size() - pos, &ch);
                CHECK(used > 0);
                pos += static_cast<size_t>(used);
                CHECK(pos + static_cast<size_t>(ch.nn_n_bytes) + static_cast<size_t>(ch.n_bytes_latent) <= bs.size());
                n_values += check_coolchic(ch, bs.data() + pos, static_cast<size_t>(ch.nn_n_bytes));
                ++n_cc;
                pos += static_cast<size_t>(ch.nn_n_bytes) + static_cast<size_t>(ch.n_bytes_latent);
            }
        }
        CHECK(pos == bs.size());
    }
    std::printf("nnquant_host_check: %d cool-chics of %d streams, %ld integers: ok\n", n_cc, argc - 1, n_values);
    return n_cc > 0 ? 0 : 1;
}
