"""Cool-chics whose OWN shape takes them to the float-path code the reference-encoded fixtures never reach (DESIGN.md section
2, "Instantiation -> test"): the fused synthesis kernel (ccd_synth_fused.hip::syn_fused_kernel<CP, C>) with k = 1, 5, 7 in a
conv position, halo up to 9, three conv layers, non-residual conv layers, relu0 = 0 / relu1 = 1, with and without the linear stabiliser, 1 .. 16 dense
channels; the generic per-layer kernel (ccd_float.hip::syn_layer_kernel) with one layer, a k x k first layer, channel counts that
change inside the conv layers, seven layers, k = 9 and 15, 1 and 6 output channels; both branches of upsample_generic_one
(ups_k_size != 8, ups_preconcat_k_size != 7) alone and next to the k = 8 / k = 7 fast paths, reading the float stack and the int8
latent; the integer planes behind such networks.

Manufactured with this repo's writer: the header by writer.derive_arch from the header of a reference-encoded fixture; the
parameter groups whose size the new header keeps are the donor's (ARM and IFCE grown to another level count by
writer.adapt_network's rules); the upsampling filters and the synthesis weights and biases (groups 4, 6, 7) of another size are
drawn, seeded, from the donor's own integers of that group, so their magnitudes stay those of a trained network.  Latents:
tests/float_matrix.py's seeded Laplace grids with -64 and 63 planted.  Shared by the CPU and GPU tests of
tests/test_synth_arch.py; every stream and every oracle result is made once per process."""
import zlib
from collections import namedtuple

import numpy as np

import float_matrix as fm

LIN, RES = 0, 1      # syn_layer.mode
NONE, RELU = 0, 1    # syn_layer.non_linearity

RGB, HOP2, HOP4, LOP5, CR = ("rgb192", 0), ("vid3_hop", 2), ("vid3_hop", 1), ("vid5", 3), ("cr192", 0)
YUV420, YUV444 = ("yuv420_8b", 0), ("yuv444_10b", 0)
EXPECTED_C = {RGB: 3, HOP2: 2, HOP4: 4, LOP5: 5, CR: 3, YUV420: 3, YUV444: 3}

# dense-grid sizes every architecture runs at (tests/float_matrix.py: one row and one column past the 64 x 32 tile / smaller than
# every halo, most k = 15 taps clamped / exact multiples of the tiles); 4:2:0 planes need even sizes: the next even ones
SIZES = [(33, 65), (7, 9), (64, 128)]
SIZES_420 = [(34, 66), (8, 10), (64, 128)]
HALO9_SIZE = (15, 47)  # one past the 14 x 46 interior of the fused synthesis kernel's tile at halo 9
UPS_PAIRS = [(4, 3), (6, 5), (10, 1), (14, 15), (8, 3), (4, 7)]  # (ups_k_size, ups_preconcat_k_size)


def _head(c, n=8, nl0=RELU, nl1=NONE):
    return [(n, 1, LIN, nl0), (c, 1, LIN, nl1)]


def _k5(c):
    return _head(c) + [(c, 5, RES, RELU), (c, 7, LIN, NONE)]


# One row per architecture.  `syn`: the kernel that computes the synthesis when the fused float kernel does not take the stream -
# "fused" = syn_fused_kernel (ccd_batch_slot_kernels & 2), "generic" = syn_layer_kernel (& 2 and & 4 clear).  `fdec`: whether
# the fused float kernel (& 4) takes the stream with CCD_OPT_FUSED_DEC = 1 / 2 (ccd_batch_plan.cpp::layout_fused_dec: 5 .. 9
# levels, 8 / 7 upsampling filters, two 1 x 1 layers then only 3 x 3 layers on C channels, C = 2 .. 5; common randomness: C = 3
# and form 2 only).  Both are STATED here, per architecture, and asserted per slot: a case that changed path fails.
# `lines`: the lines of the matrix the row stands for (the inventory test asserts the set).
Arch = namedtuple("Arch", "name donor layers ups levels stab fmt syn fdec lines extra_sizes")


def _arch(name, donor, layers, lines, syn, fdec, ups=(8, 7), levels=None, stab=None, fmt="own", extra_sizes=()):
    return Arch(name, donor, layers, ups, levels, stab, fmt, syn, fdec, tuple(lines), tuple(extra_sizes))


ARCHS = [
    # ---- the fused synthesis kernel by the network's own shape ----
    _arch("k5k7", RGB, _k5(3), ["k5", "k7", "conv-linear", "C3", "rgb8-planes"], "fused", False),
    _arch("halo9", RGB, _head(3) + [(3, 7, RES, NONE)] * 3, ["halo9", "nconv3"], "fused", False, extra_sizes=[HALO9_SIZE]),
    _arch("nconv3", RGB, _head(3) + [(3, 3, LIN, RELU), (3, 3, RES, NONE), (3, 3, LIN, NONE)], ["nconv3-k3"], "fused", True),
    _arch("k1conv", RGB, _head(3) + [(3, 1, RES, NONE)], ["k1"], "fused", False),
    _arch("two1x1", RGB, _head(3, nl0=NONE, nl1=RELU), ["relu0=0 relu1=1"], "fused", True),
    _arch("hidden1", RGB, _head(3, n=1) + [(3, 5, RES, NONE)], ["N1"], "fused", False),
    _arch("hidden127", RGB, _head(3, n=127) + [(3, 5, RES, NONE)], ["N127"], "fused", False),
    _arch("nostab", RGB, _k5(3), ["stab0"], "fused", False, stab=0),
    _arch("stab", RGB, _head(3) + [(3, 5, LIN, RELU)], ["stab1"], "fused", False, stab=1),
    _arch("c2", HOP2, _k5(2), ["C2"], "fused", False),
    _arch("c4", HOP4, _k5(4), ["C4"], "fused", False),
    _arch("c5", LOP5, _k5(5), ["C5"], "fused", False),
    _arch("lv1", RGB, _k5(3), ["levels1"], "fused", False, levels=1),
    _arch("lv2", RGB, _k5(3), ["levels2"], "fused", False, levels=2),
    _arch("lv4", RGB, _k5(3), ["levels4"], "fused", False, levels=4),
    _arch("cr7", CR, _k5(3), ["cr14"], "fused", False, levels=7),
    _arch("cr8", CR, _k5(3), ["cr16"], "fused", False, levels=8),
    _arch("cr9", CR, _k5(3), ["cr18"], "generic", False, levels=9),
    # ---- the generic layer kernel by the network's own shape ----
    _arch("one", RGB, [(3, 1, LIN, NONE)], ["g-one"], "generic", False),
    _arch("first3", RGB, [(8, 3, LIN, RELU), (3, 1, LIN, NONE)], ["g-first-k3"], "generic", False),
    _arch("l1wide", RGB, [(16, 1, LIN, RELU), (8, 1, LIN, RELU), (3, 3, LIN, NONE)], ["g-l1"], "generic", False),
    _arch("seven", RGB, [(12, 1, LIN, RELU), (6, 1, LIN, RELU), (6, 3, RES, RELU), (4, 3, LIN, RELU), (4, 5, RES, NONE), (5, 1, LIN, RELU),
                         (3, 9, LIN, NONE)], ["g-seven"], "generic", False),
    _arch("k15", RGB, [(4, 1, LIN, RELU), (3, 15, LIN, NONE)], ["g-k15"], "generic", False),
    _arch("out1", RGB, [(8, 1, LIN, RELU), (1, 3, LIN, NONE)], ["g-out1"], "generic", False, fmt="float"),
    _arch("out6", RGB, [(8, 1, LIN, RELU), (6, 1, LIN, NONE), (6, 3, RES, NONE)], ["g-out6"], "generic", False, fmt="float"),
    # ---- integer planes behind a k = 5 architecture (8-bit RGB: "k5k7" above) ----
    _arch("p420", YUV420, _k5(3), ["yuv420-8-planes"], "fused", False),
    _arch("p444", YUV444, _k5(3), ["yuv444-10-planes"], "fused", False),
]
# ---- upsampling: the donor's synthesis behind other filters, on 7 levels (the transposed convolution reads the float stack from
# the second step on) and on 2 (its only step reads the int8 latent) ----
for _u, _p in UPS_PAIRS:
    ARCHS.append(_arch(f"ups{_u}x{_p}", RGB, None, [f"ups{_u}/{_p} levels7"], "fused", False, ups=(_u, _p)))
    ARCHS.append(_arch(f"ups{_u}x{_p}lv2", RGB, None, [f"ups{_u}/{_p} levels2"], "fused", False, ups=(_u, _p), levels=2))

# the matrix of shapes to cover, line by line: the inventory test asserts that the rows above cover exactly this
MATRIX = ({"k5", "k7", "conv-linear", "halo9", "nconv3", "nconv3-k3", "k1", "relu0=0 relu1=1", "N1", "N127", "stab0", "stab1", "C2", "C3",
           "C4", "C5", "levels1", "levels2", "levels4", "cr14", "cr16", "cr18", "g-one", "g-first-k3", "g-l1", "g-seven", "g-k15",
           "g-out1", "g-out6", "yuv420-8-planes", "yuv444-10-planes", "rgb8-planes"}
          | {f"ups{u}/{p} levels{n}" for u, p in UPS_PAIRS for n in (7, 2)})
# ccd_latent_footprint by impulse: (8, 7) behind k = 5 and k = 7 layers, four other filter pairs, and the motion donor (its
# synthesis output goes through the nearest final resize) at (6, 5); picture sizes
FOOTPRINT_ARCHS = ["k5k7", "ups4x3", "ups6x5", "ups10x1", "ups14x15"]
FOOTPRINT_MOTION = _arch("motion6x5", HOP2, None, [], "fused", False, ups=(6, 5))
FOOTPRINT_SIZES = [(97, 161), (7, 9)]
# one architecture per class that also runs alone in a batch (at 33 x 65)
ALONE = ["k5k7", "halo9", "c5", "lv1", "cr8", "cr9", "seven", "out1", "ups14x15", "ups4x7lv2", "p420", "p444"]

# label = "<architecture> dense=<h>x<w>"; .levels / .c / .cr / .picture / .label are what float_matrix.describe reads
Case = namedtuple("Case", "label arch_name spec donor cc levels dense c cr picture bitdepth frame_data_type triple stream latents arch")

_CASES = None
_MADE = {}
_REF = {}
_PLANES = {}


def _latents(arch, label):
    """float_matrix's seeded Laplace latents; where every grid is too small for its few forced entries to hold both ends of the
    alphabet, the first entries of other grids take the missing ones (tests/float_tail.py)."""
    lat = fm._latents(arch, label)
    for v in (-64, 63):
        if not any((a == v).any() for a in lat):
            a = next(a for a in lat if a.flat[0] not in (-64, 63))
            a.flat[0] = v
    return lat


def network(donor, ints, arch, label):
    """Quantised parameters for `arch`: the donor's groups where the size is unchanged; ARM and IFCE (and, when only the level
    count changed, the filters and the synthesis) by writer.adapt_network's rules, applied to the donor's own architecture at the
    new geometry; groups 4, 6, 7 (ups.w, syn.w, syn.b) of another size drawn from the donor's integers of that group."""
    from cool_chic_amd import writer

    twin = writer.derive_arch(arch, syn_layers=[(l.out_ft, l.k_size, l.mode, l.non_linearity) for l in donor.syn_layer[:donor.n_layer_synthesis]],
                              ups_k_size=donor.ups_k_size, ups_preconcat_k_size=donor.ups_preconcat_k_size,
                              linear_stabiliser_synth=donor.linear_stabiliser_synth)
    dl, tl, al = writer.network_layout(donor), writer.network_layout(twin), writer.network_layout(arch)
    grown = np.split(writer.adapt_network(donor, ints, twin), np.cumsum(tl)[:-1])
    own = np.split(np.asarray(ints, np.int64), np.cumsum(dl)[:-1])
    rng = np.random.default_rng(zlib.crc32(("network " + label).encode()))
    out = []
    for k in range(8):
        if al[k] == tl[k]:
            out.append(grown[k])
        else:
            assert k in (4, 6, 7) and dl[k] > 0, (label, k, dl[k], tl[k], al[k])
            out.append(rng.choice(own[k], size=al[k]))
    return np.concatenate(out).astype(np.int32)


def derive(donor, spec, size, img_size=None):
    """(header, level count) of `spec` on `donor` with dense grid `size` (the picture: size << lo), or with picture `img_size`."""
    from cool_chic_amd import writer

    lo = donor.latent_resolution[0]
    n = spec.levels if spec.levels is not None else donor.latent_resolution[1] - donor.latent_resolution[0] + 1
    hi = lo + n - 1
    if img_size is None:
        img_size = (size[0] << lo, size[1] << lo)
    else:
        size = (-(-img_size[0] // (1 << lo)), -(-img_size[1] // (1 << lo)))
    changes = dict(img_size=tuple(img_size), latent_resolution=(lo, hi), n_latent_grids=n,
                   ups_k_size=spec.ups[0], ups_preconcat_k_size=spec.ups[1])
    if donor.flag_hyperlatent:
        changes["hyperlatent_resolution"] = (min(4, hi), hi)
        changes["n_latent_grids"] = n + hi - min(4, hi) + 1
    if spec.layers is not None:
        changes["syn_layers"] = spec.layers
    if spec.stab is not None:
        changes["linear_stabiliser_synth"] = spec.stab
    arch = writer.derive_arch(donor, **changes)
    g0 = next(g for g in range(arch.n_grids) if not arch.is_hyperlatent[g])
    assert (arch.grid_h[g0], arch.grid_w[g0]) == tuple(size), (spec.name, size)
    return arch, n


def footprint_case(load_golden, oracle, spec, img_size):
    """(label, header, NN payload, latents) of `spec` at a PICTURE size, for the impulse test of ccd_latent_footprint."""
    from cool_chic_amd import writer

    name, k = spec.donor
    donor, ints, _ = fm._donor(load_golden, oracle, name, k)
    arch, _ = derive(donor, spec, None, img_size=img_size)
    label = f"{spec.name} picture={img_size[0]}x{img_size[1]}"
    nn = writer.encode_network(arch, network(donor, ints, arch, spec.name))
    return label, arch, nn, _latents(arch, label)


def make(load_golden, oracle, spec, size):
    from cool_chic_amd import writer

    key = (spec.name, tuple(size))
    if key in _MADE:
        return _MADE[key]
    name, k = spec.donor
    donor, ints, fh = fm._donor(load_golden, oracle, name, k)
    arch, n = derive(donor, spec, size)
    label = f"{spec.name} dense={size[0]}x{size[1]}"
    # (the network is the architecture's, not the size's: seeded by the architecture's name)
    nn = writer.encode_network(arch, network(donor, ints, arch, spec.name))  # (also sets the payload size in `arch`)
    lat = _latents(arch, label)
    c, cr = int(arch.out_channels), bool(arch.flag_common_randomness)
    picture = spec.fmt == "own" and c == 3
    if picture:
        # the I frame of a video fixture is 4:2:0 there; a three-channel donor from a video goes in as 8-bit RGB
        bitdepth, fdt = (int(fh.bitdepth), int(fh.frame_data_type)) if name in ("rgb192", "cr192", "yuv420_8b", "yuv444_10b") else (8, 0)
        stream = writer.encode_stream(writer.cc_header_bytes(arch), nn, lat, bitdepth=bitdepth, frame_data_type=fdt)
        (_fh, (triple,)), = oracle.split_stream(stream)[1]
    else:
        bitdepth, fdt, stream = 0, int(fh.frame_data_type), None
        blob = writer.encode_coolchic(arch, nn, lat)
        h = writer.parse_cc_header(blob)
        a, b = h.n_bytes_header, h.n_bytes_header + h.nn_n_bytes
        assert len(blob) == b + h.n_bytes_latent, label
        triple = (blob[:a], blob[a:b], blob[b:])
    _MADE[key] = Case(label, spec.name, spec, name, k, n, tuple(size), c, cr, picture, bitdepth, fdt, triple, stream, lat, arch)
    return _MADE[key]


def sizes_of(spec):
    return (SIZES_420 if spec.donor == YUV420 else SIZES) + list(spec.extra_sizes)


def cases(load_golden, oracle):
    """Every case, in the order the batches hold them."""
    global _CASES
    if _CASES is None:
        _CASES = [make(load_golden, oracle, spec, size) for spec in ARCHS for size in sizes_of(spec)]
    return _CASES


def reference(oracle, case):
    """oracle.decode_coolchic of the case (latent, dense, syn_out, out), once per process; treat as read-only."""
    if case.label not in _REF:
        r = oracle.decode_coolchic(*case.triple)
        _REF[case.label] = {k: r[k] for k in ("n_grids", "latent", "dense", "syn_out", "out")}
    return _REF[case.label]


def reference_planes(oracle, case):
    """Integer planes of a picture case: oracle.decode_video of its one-frame stream, once per process."""
    if case.label not in _PLANES:
        _PLANES[case.label] = oracle.decode_video(case.stream)[0]["planes"]
    return _PLANES[case.label]


def expected_kernels(case, form, forced_generic=False):
    """(ccd_batch_slot_kernels & 2: the fused synthesis kernel, & 4: the fused float kernel) the slot must report with
    CCD_OPT_FUSED_DEC = form - from the case table alone."""
    if forced_generic:
        return False, False
    fdec = case.spec.fdec and form != 0 and not (case.cr and form != 2)
    # (the fused float kernel replaces the whole float path: a slot it takes does not report the fused synthesis kernel)
    return (case.spec.syn == "fused" and not fdec), fdec


def facts(arch):
    """What an architecture exercises of {k in 1, 5, 7 in a conv position, a non-residual conv layer, three conv layers, CP 4, CP
    16, no stabiliser, ups_k != 8, pre_k != 7}: the set of those that hold for a parsed header."""
    L = [arch.syn_layer[i] for i in range(arch.n_layer_synthesis)]
    conv = L[2:]
    n_levels = sum(1 for g in range(arch.n_grids) if not arch.is_hyperlatent[g])
    out = set()
    for l in conv:
        if l.k_size in (1, 5, 7):
            out.add(f"conv k={l.k_size}")
        if l.mode != RES:
            out.add("conv linear")
    if len(conv) == 3:
        out.add("n_conv 3")
    cp = (arch.input_feature_synthesis + 3) // 4 * 4
    if cp in (4, 16):
        out.add(f"CP {cp}")
    if not arch.linear_stabiliser_synth:
        out.add("no stabiliser")
    if n_levels > 1 and arch.ups_k_size != 8:
        out.add("ups_k != 8")
    if n_levels > 1 and arch.ups_preconcat_k_size != 7:
        out.add("pre_k != 7")
    return out


ALL_FACTS = {"conv k=1", "conv k=5", "conv k=7", "conv linear", "n_conv 3", "CP 4", "CP 16", "no stabiliser", "ups_k != 8", "pre_k != 7"}
