"""Inputs of tests/test_producer_output_tail.py: networks on which a wrong sum over a pixel's lanes in the producers' output
layer (ccd_entropy_pipe.hip, producer_grid: the output layer runs on the activations each lane holds and is reduced over the
pixel's lane group) shows in the table indices.

In the hidden layers a lane whose units lie past the layer (o = q + lanes t >= dim) computes a copy of unit dim - 1.  The
networks here make that copy expensive to let in: unit dim - 1 of the layer in front of the output layer gets a large positive
bias (it is active at every pixel) and both output rows weight it heavily, so one extra copy moves mu and the log-scale by many
table steps.  Architectures are derived from kodim14's cool-chic (tests/producer_cases.py edits the same donor), parameters
drawn as tests/arm_layouts.py draws them, streams written with this repo's writer; every stream and oracle result is made once
per process."""
from collections import namedtuple

import numpy as np

import producer_cases as pc
from arm_layouts import draw_network

IMG_SIZE = (32, 320)  # grids 0 / 1 / 2 = 32 x 320, 16 x 160, 8 x 80: 8-, 4- and 2-pixel tasks
# (spatial contexts, IFCE features, hidden layers): dim 20 with 2 / 1 / 0 hidden layers (the output layer behind a hidden layer,
# behind the first layer, behind the raw inputs; 14 + 6 with two hidden layers is the compile-time shape), an odd dim (19), a
# dim that does not fill its last 4-vector (22, 6), dim 30 (the widest instantiations of the pipelined kernel: four units per
# lane on 8-pixel tasks), and dim 64 (the generic kernel's side of the 64-input border; one hidden
# layer: with two the generic kernel's LDS need is past what DecodeBatch takes, arm_layouts.device_decodable)
SHAPES = [(14, 6, 2), (14, 6, 1), (14, 6, 0), (13, 6, 2), (13, 6, 0), (16, 6, 1), (4, 2, 2), (24, 6, 2), (40, 24, 1)]
# in the network's integers (kodim14's trained ARM: |weight| <= 202, median 26; |bias| <= 73): large next to the trained values,
# small enough that mu and the log-scale stay inside their tables (a saturated index would hide an extra copy)
UNIT_BIAS = 64      # bias of the exposed unit
UNIT_WEIGHT = 48    # its weight in the mu row; -UNIT_WEIGHT in the log-scale row

Case = namedtuple("Case", "name shape arch fh stream triple latents planes mu_scale_idx control_idx doubled_idx")

_CASES = {}
_DONOR = None


def donor(oracle):
    """(frame header, parsed cool-chic header, network integers) of kodim14."""
    global _DONOR
    if _DONOR is None:
        from conftest import load_golden
        from cool_chic_amd import writer

        bs, z, _ = load_golden("kodim14")
        (fh, ccs), = oracle.split_stream(bs)[1]
        _DONOR = (fh, writer.parse_cc_header(ccs[0][0]), np.array(z["cc0.nn_ints"]))
    return _DONOR


def name_of(shape):
    return "s%d_i%d_h%d" % shape


def expose_last_unit(arch, ints, weight=UNIT_WEIGHT):
    """The network's integers with unit dim - 1 in front of the output layer exposed: bias UNIT_BIAS (a network without hidden
    layer has no such bias: the unit is the last input, an IFCE feature) and output weights +-`weight`."""
    from cool_chic_amd import writer

    g = np.split(np.asarray(ints, dtype=np.int64).copy(), np.cumsum(writer.network_layout(arch))[:-1])
    dim, n_hidden = arch.total_context_arm, arch.n_hidden_layers_arm
    if n_hidden > 0:
        g[1][(n_hidden - 1) * dim + dim - 1] = UNIT_BIAS
    out = g[0][n_hidden * dim * dim: n_hidden * dim * dim + 2 * dim].reshape(2, dim)  # [row][input], rows mu / log-scale
    out[0, dim - 1] = weight
    out[1, dim - 1] = -weight
    return np.concatenate(g).astype(np.int32)


def _indices(oracle, triple):
    r = oracle.decode_coolchic(*triple, stop_after_entropy=True)
    return r, [np.array(ms) for ms in r["mu_scale_idx"]]


def case(oracle, shape):
    """The stream of one shape (crafted latents of producer_cases), the oracle's latents, integer planes and table indices, and
    the table indices the same latents get when the exposed unit's two output weights are zero (the control) and when they
    are doubled (what one extra copy of the unit in the sum amounts to)."""
    if shape not in _CASES:
        from cool_chic_amd import writer

        fh, hdr, ints = donor(oracle)
        n_sp, n_if, n_hidden = shape
        arch = writer.derive_arch(hdr, spatial_context_arm=n_sp, n_hidden_layers_arm=n_hidden, output_feature_ifce=n_if, img_size=IMG_SIZE)
        assert arch.total_context_arm == n_sp + n_if
        drawn = draw_network(hdr, ints, arch, np.random.default_rng(8100 + 100 * n_sp + 10 * n_if + n_hidden))
        latents = pc.crafted_latents(arch)

        def encode(net):
            nn = writer.encode_network(arch, net)
            s = writer.encode_stream(writer.cc_header_bytes(arch), nn, latents, bitdepth=fh.bitdepth, frame_data_type=fh.frame_data_type)
            return s, oracle.split_stream(s)[1][0][1][0]

        stream, triple = encode(expose_last_unit(arch, drawn))
        ref, idx = _indices(oracle, triple)
        _, control = _indices(oracle, encode(expose_last_unit(arch, drawn, weight=0))[1])
        _, doubled = _indices(oracle, encode(expose_last_unit(arch, drawn, weight=2 * UNIT_WEIGHT))[1])
        planes = [np.array(p) for p in oracle.decode_video(stream)[0]["planes"]]
        _CASES[shape] = Case(name_of(shape), shape, arch, fh, stream, triple, [np.array(a) for a in ref["latent"]], planes, idx, control, doubled)
    return _CASES[shape]


Crafted = namedtuple("Crafted", "size arch fh triple latents planes")
_CRAFTED = {}


def crafted(oracle, size):
    """kodim14's own networks on a picture of `size` with producer_cases.crafted_latents: the stream's cool-chic, the oracle's
    latents and integer planes."""
    if size not in _CRAFTED:
        from conftest import load_golden
        from cool_chic_amd import writer

        fh, hdr, _ = donor(oracle)
        nn = oracle.split_stream(load_golden("kodim14")[0])[1][0][1][0][1]
        arch = writer.derive_arch(hdr, img_size=size)
        assert writer.network_layout(arch) == writer.network_layout(hdr)
        stream = writer.encode_stream(writer.cc_header_bytes(arch), nn, pc.crafted_latents(arch), bitdepth=fh.bitdepth,
                                      frame_data_type=fh.frame_data_type)
        triple = oracle.split_stream(stream)[1][0][1][0]
        ref = oracle.decode_coolchic(*triple, stop_after_entropy=True)
        planes = [np.array(p) for p in oracle.decode_video(stream)[0]["planes"]]
        _CRAFTED[size] = Crafted(size, arch, fh, triple, [np.array(a) for a in ref["latent"]], planes)
    return _CRAFTED[size]
