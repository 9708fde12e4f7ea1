"""Cool-chics whose ARM and IFCE LAYOUT the reference encoder's presets never have: odd and 1-wide ARMs,
0 .. 7 hidden layers, more than 64 inputs (the encoder kernels' dynamic-LDS opt-in), IFCE on coarse, hyperlatent and the last
grid, and pictures of 10 .. 256 symbols around the 64-symbol chunks of the device range coder.  Manufactured with this repo's
writer: architecture derived from the reference-encoded `rgb192` fixture, ARM / IFCE parameters drawn (seeded) from the value
distribution of its trained ones (`build_stream`, the rule tests/golden/gen/make_arm_sweep.py wrote arm_sweep.npz with), its
latent pyramid tiled to the new size or seeded symbols with -64 next to 63.  The yardsticks are the CPU oracle and the host
writer.  Shared by the CPU and GPU tests of tests/test_arm_layouts.py and the geometry tests of tests/test_rdoq.py; every
stream and every oracle result is made once per process."""
from collections import namedtuple

import numpy as np

SWEEP_IMG_SIZE = (32, 320)
# (spatial contexts, IFCE features, hidden layers): dim 71 / 65 / 70 / 64 (= exactly 64 KB of LDS in the encoder kernels) / 1 /
# 32 / 5 / 9
ARM_SHAPES = [(40, 31, 7), (40, 25, 1), (39, 31, 0), (40, 24, 2), (1, 0, 0), (1, 31, 7), (3, 2, 4), (2, 7, 5)]
# ifce_resolution -> input_features_ifce of rgb192's ten grids: (0, 15) [9 8 7 6 5 4 3 2 1 1] (the last grid: one all-zero
# channel), (3, 15) [0 0 0 6 5 4 3 2 1 1], (1, 1) [0 8 0 ..], (4, 4) [0 0 0 0 5 4 0 ..] (a latent grid and the hyperlatent grid
# of the same level)
PLACEMENTS = [(0, 15), (3, 15), (1, 1), (4, 4)]
PLACEMENT_SHAPES = [(6, 3, 3), (9, 7, 6)]  # an odd dim; 7 features (and the two hidden-layer counts ARM_SHAPES lacks)
PLACEMENT_SIZES = [(18, 65), (37, 100)]
# n_symbols 10, 63, 64, 64, 65, 65, 127, 128, 255, 256 with rgb192's ten grids
TINY_SIZES = [(1, 1), (5, 8), (1, 29), (2, 19), (1, 30), (3, 13), (2, 40), (3, 27), (8, 23), (5, 34)]
TINY_SHAPES = [((5, 2, 1), (0, 15)), ((6, 0, 2), None)]  # IFCE on every grid / no IFCE
# the tiny cases' seeds, found by a search over 0 .. 63 per case so that among them the range coder seals with one and with two
# words, resolves inverted runs with and without a carry and holds a run of two words (test_chain_inventory asserts it)
TINY_SEEDS = {"tiny5x8_s5_i2_h1": 13, "tiny1x29_s5_i2_h1": 16, "tiny2x19_s6_i0_h2": 32, "tiny1x30_s5_i2_h1": 28, "tiny2x40_s6_i0_h2": 33,
              "tiny5x34_s6_i0_h2": 26}  # these six seal with two words (63, 64, 64, 65, 127 and 256 symbols)

# the other cases' seeds where the first draw (7000 + index / 7100 + index) gave a network that does not answer to one of its
# last parameters, e.g. a last hidden unit that is never positive (test_last_parameters_are_visible_in_the_bytes): the first of
# seed + 100 j that does
LAYOUT_SEEDS = {"arm_s40_i31_h7": 9400, "arm_s40_i25_h1": 7601, "arm_s40_i24_h2": 7703, "arm_s1_i31_h7": 7405, "arm_s3_i2_h4": 7106,
                "ifce0_15_18x65_s9_i7_h6": 11001, "ifce0_15_37x100_s6_i3_h3": 7202, "ifce3_15_18x65_s6_i3_h3": 7404,
                "ifce3_15_18x65_s9_i7_h6": 7405, "ifce3_15_37x100_s6_i3_h3": 7306, "ifce3_15_37x100_s9_i7_h6": 7207,
                "ifce1_1_37x100_s9_i7_h6": 7211, "ifce4_4_37x100_s6_i3_h3": 7214}

Case = namedtuple("Case", "name kind shape placement img_size arch hdr nn payload cc stream latents")

_DONOR = None
_CASES = None
_ENTROPY = {}
_CHAIN = {}


def draw_network(donor, donor_ints, arch, rng):
    """Quantised parameters for `arch`: ARM and IFCE values drawn from the donor's trained ones of the same kind, the float
    path (upsampling, synthesis) the donor's, unchanged."""
    from cool_chic_amd import writer

    dim = arch.total_context_arm
    dl, al = writer.network_layout(donor), writer.network_layout(arch)
    d = np.split(np.asarray(donor_ints, dtype=np.int64), np.cumsum(dl)[:-1])
    out = []
    for k in range(8):
        if k >= 4:  # upsampling / synthesis: the donor's trained float path, unchanged
            assert al[k] == dl[k]
            out.append(d[k])
        elif al[k] == 0:
            out.append(np.zeros(0, np.int64))
        else:
            # values drawn from the trained parameters of the same kind; hidden-layer weights shrink with the width so that the
            # residual layers keep activations (and so mu / scale) in the trained range
            v = rng.choice(d[k], size=al[k]).astype(np.float64)
            if k == 0:
                v *= 0.2 * min(1.0, (donor.total_context_arm / dim) ** 0.5)
            if k == 1:  # arm.b = hidden layers, output layer (mu, log-scale), stabiliser: the trained output biases keep the
                # predicted distributions (and so the stream sizes) near the donor's
                n_tail = 4 if arch.linear_stabiliser_arm else 2
                v[-n_tail:] = d[k][-n_tail:]
            out.append(np.round(v).astype(np.int64))
    return np.concatenate(out).astype(np.int32)


def build_stream(donor, donor_ints, latents, dim, n_hidden, n_ifce, seed, img_size=SWEEP_IMG_SIZE, ifce_resolution=None,
                 make_latents=None):
    """One-intra-frame stream with `dim` ARM inputs (dim - n_ifce spatial contexts), `n_hidden` hidden layers, IFCE off
    (n_ifce = 0) or on the grid pairs `ifce_resolution` selects (None: the donor's); returns (stream, latents, network integers).
    The latents are the donor's `latents` tiled to `img_size`, or make_latents(arch)."""
    from cool_chic_amd import writer

    rng = np.random.default_rng(seed)
    changes = dict(spatial_context_arm=dim - n_ifce, n_hidden_layers_arm=n_hidden, output_feature_ifce=n_ifce, img_size=tuple(img_size))
    if n_ifce == 0:
        changes.update(has_ifce_resolution=0)
    elif ifce_resolution is not None:
        changes.update(has_ifce_resolution=1, ifce_resolution=tuple(ifce_resolution))
    arch = writer.derive_arch(donor, **changes)
    assert arch.total_context_arm == dim
    ints = draw_network(donor, donor_ints, arch, rng)
    nn = writer.encode_network(arch, ints)
    lat = writer.tile_latents(latents, donor, arch) if make_latents is None else make_latents(arch)
    stream = writer.encode_stream(writer.cc_header_bytes(arch), nn, lat, bitdepth=8, frame_data_type=0)
    return stream, lat, ints


def extreme_latents(arch, seed):
    """Symbols -64 and 63 next to each other (checkerboard patches) inside otherwise Laplacian grids
    (test_device_encoder.py::_extreme_latents, seeded per case)."""
    rng = np.random.default_rng(seed)
    out = []
    for g in range(arch.n_grids):
        h, w = arch.grid_h[g], arch.grid_w[g]
        a = np.clip(np.round(rng.laplace(size=(h, w)) * 3), -64, 63).astype(np.int8)
        yy, xx = np.mgrid[0:h, 0:w]
        patch = ((yy // 7 + xx // 5) % 3 == 0)
        a[patch] = np.where((yy + xx) % 2 == 0, -64, 63).astype(np.int8)[patch]
        out.append(a)
    return out


def donor():
    """(parsed header, network integers, latent grids) of rgb192's cool-chic."""
    global _DONOR
    if _DONOR is None:
        from conftest import load_golden
        from cool_chic_amd import writer
        from oracle import oracle_py

        bs, z, _ = load_golden("rgb192")
        hdr, _, _ = oracle_py.split_stream(bs)[1][0][1][0]
        h = writer.parse_cc_header(hdr)
        _DONOR = (h, np.asarray(z["cc0.nn_ints"]), [np.asarray(z[f"cc0.latent{g}"]) for g in range(h.n_grids)])
    return _DONOR


def specs():
    """[(name, kind, (spatial, IFCE out, hidden), ifce_resolution or None, (H, W), seed, extreme latents?)], about 50."""
    out = []
    for i, shape in enumerate(ARM_SHAPES):
        out.append(("arm_s%d_i%d_h%d" % shape, "arm", shape, (0, 2) if shape[1] else None, (18, 65), 7000 + i, i in (0, 6)))
    k = 0
    for res in PLACEMENTS:
        for size in PLACEMENT_SIZES:
            for shape in PLACEMENT_SHAPES:
                name = "ifce%d_%d_%dx%d_s%d_i%d_h%d" % (res + size + shape)
                out.append((name, "placement", shape, res, size, 7100 + k, size == (18, 65) and shape == PLACEMENT_SHAPES[1]))
                k += 1
    for size in TINY_SIZES:
        for shape, res in TINY_SHAPES:
            name = "tiny%dx%d_s%d_i%d_h%d" % (size + shape)
            out.append((name, "tiny", shape, res, size, TINY_SEEDS.get(name, 0), True))
    return [(s[0],) + s[1:5] + (LAYOUT_SEEDS.get(s[0], s[5]),) + s[6:] for s in out]


def make_case(spec):
    from cool_chic_amd import writer
    from oracle import oracle_py

    name, kind, (n_sp, n_if, n_hidden), res, size, seed, extreme = spec
    d_hdr, d_ints, d_lat = donor()
    stream, lat, _ = build_stream(d_hdr, d_ints, d_lat, n_sp + n_if, n_hidden, n_if, seed, img_size=size, ifce_resolution=res,
                                  make_latents=(lambda a: extreme_latents(a, seed + 1)) if extreme else None)
    (_fh, ccs), = oracle_py.split_stream(stream)[1]
    hdr, nn, payload = ccs[0]
    lat = [np.ascontiguousarray(a, dtype=np.int8) for a in lat]
    return Case(name, kind, (n_sp, n_if, n_hidden), res, size, writer.parse_cc_header(hdr), hdr, nn, payload, hdr + nn + payload, stream, lat)


def cases():
    global _CASES
    if _CASES is None:
        _CASES = [make_case(s) for s in specs()]
    return _CASES


def case(name):
    return next(c for c in cases() if c.name == name)


def entropy(oracle, c):
    """The oracle's entropy decode of a case (latents, (mu, scale) table indices in decode order, ..), once."""
    if c.name not in _ENTROPY:
        _ENTROPY[c.name] = oracle.decode_coolchic(c.hdr, c.nn, c.payload, stop_after_entropy=True)
    return _ENTROPY[c.name]


def has_sources(arch, g):
    """Grid g's features read coarser grids (on the last grid the stack is one all-zero channel: the feature is its bias)."""
    return arch.input_features_ifce[g] > 0 and g != arch.n_grids - 1


def device_decodable(arch):
    """Whether DecodeBatch takes this ARM: below 64 inputs the pipelined entropy kernel serves every shape here; from 64 on the
    generic kernel keeps the whole ARM in LDS and ccd_batch_add refuses what needs more than 160 KB with CCD_ERR_UNSUPPORTED
    (ccd_entropy.hip::entropy_lds_bytes, restated: the ARM, two activation columns per pixel of a 64-pixel chunk, the chunk's
    CDF windows and bookkeeping)."""
    dim, n_layers = arch.total_context_arm, arch.n_hidden_layers_arm + 1
    if dim < 64:
        return True
    arm_len = (n_layers - 1) * (dim * dim + dim) + 2 * (2 * dim + 2)
    lds = ((arm_len + 1) & ~1) * 8 + (2 * dim * 64 + 2 * 64) * 8 + 64 * 128 * 4 + (4 * 64 + 4) * 4 + 64 * 8
    return lds <= 160 * 1024


# ---- the range encoder with counters ----------------------------------------------------------------------------------
ChainCount = namedtuple("ChainCount", "payload words runs carry plain longest seal_words")
M64 = (1 << 64) - 1


def chain_count(intervals):
    """constriction's RangeEncoder (tests/golden/gen/shims/constriction/stream/queue.py) over [(left, right)] out of 2^24, with
    the counters of ccd_enc_slot_status: words written, inverted runs begun, runs resolved with / without a carry (the seal's
    included); and the longest run in words and whether the seal is one word or two."""
    lower, rng, inv, out = 0, M64, None, []
    runs = carry = plain = longest = 0

    def flush(c):
        nonlocal carry, plain, longest, inv
        n, first = inv
        out.append((first + 1) & 0xFFFFFFFF if c else first)
        out.extend([0 if c else 0xFFFFFFFF] * (n - 1))
        longest = max(longest, n)
        if c:
            carry += 1
        else:
            plain += 1
        inv = None

    for left, right in intervals:
        scale = rng >> 24
        rng = scale * (right - left)
        new = (lower + scale * left) & M64
        if inv is not None and ((new + rng) & M64) > new:
            flush(new < lower)
        lower = new
        if rng < (1 << 32):
            word = lower >> 32
            lower = (lower << 32) & M64
            rng = (rng << 32) & M64
            if inv is not None:
                inv = (inv[0] + 1, inv[1])
            elif ((lower + rng) & M64) > lower:
                out.append(word)
            else:
                inv = (1, word)
                runs += 1
    seal = 0
    if intervals:
        point = (lower + (1 << 32) - 1) & M64
        if inv is not None:
            flush(point < lower)
        out.append(point >> 32)
        seal = 1
        if (((lower + rng) & M64) >> 32) == point >> 32:
            out.append(0)
            seal = 2
    return ChainCount(np.asarray(out, dtype="<u4").tobytes(), len(out), runs, carry, plain, longest, seal)


_BOUNDS = {}


def coding_order_intervals(oracle, c):
    """[(left, right)] of every symbol of a case in coding order (grids last to first, each in the oracle's decode order: raster
    when W <= 9, else by (x + 10 y, y)), from the oracle's (mu, scale) indices and oracle.laplace_bounds."""
    r = entropy(oracle, c)
    out = []
    for g in range(r["n_grids"] - 1, -1, -1):
        h, w = r["grid_hw"][g]
        yy, xx = np.mgrid[0:h, 0:w]
        y, x = yy.ravel(), xx.ravel()
        order = np.arange(h * w) if w <= 9 else np.lexsort((y, x + 10 * y))
        sym = r["latent"][g].ravel()[order]
        for (m, s), v in zip(r["mu_scale_idx"][g].tolist(), sym.tolist()):
            key = (m, s, v)
            if key not in _BOUNDS:
                _BOUNDS[key] = oracle.laplace_bounds(m, s, v)
            out.append(_BOUNDS[key])
    return out


def chain(oracle, c):
    if c.name not in _CHAIN:
        _CHAIN[c.name] = chain_count(coding_order_intervals(oracle, c))
    return _CHAIN[c.name]
