"""Cool-chics for the tail of the float path (ccd_float.hip: resize_nearest_kernel, resize_interp_kernel, cr_noise_kernel with its
bicubic x2 chain, planes_kernel behind a resize): pictures whose finest latent grid is 2, 4 or 8 times
coarser than the picture (latent_resolution (lo, lo + span), lo = 1 .. 3) in the three final-resize modes, at picture sizes
that are no multiple of anything - non-integer scales, 1-pixel axes, exactly x2 on one axis only, sizes around the kernels'
block of 64 columns x 4 rows - in the four plane formats; videos whose motion cool-chics (latent_resolution (2, 6), nearest)
sit at non-integer scales; common randomness at sizes that are odd at every level.  Manufactured with this repo's writer from
the trained networks of reference-encoded fixtures and seeded latents (tests/float_matrix.py's recipe).  Shared by the CPU and
the GPU tests of tests/test_float_tail.py; every stream and every oracle result is made once per process."""
from collections import namedtuple

import numpy as np

import float_matrix as fm

MODES = ("nearest", "bilinear", "bicubic")  # final_upsampling_type 0, 1, 2
LOS = (1, 2, 3)
# format class -> donor fixture
DONORS = {"rgb8": "rgb192", "yuv420_8": "yuv420_8b", "yuv420_10": "yuv420_10b", "yuv444_10": "yuv444_10b"}
# donor -> [(lo, picture size)], each in every mode.  Dense grid = ceil(size / 2^lo).
#   1 x 13, 13 x 1: in == out on one axis only                         10 x 17, lo 1: exactly x2 on rows, general on columns
#   10 x 18, lo 1: exactly x2 on both axes                            5 x 7: below one block; lo 3: a 1 x 1 grid, every tap clamped
#   37 x 100: one column block and part of another                    65 x 18: 16 row blocks and one row
#   33 x 257: four column blocks and one column
#   4:2:0 (even sizes): 2 x 2 (a 1 x 1 grid, one chroma sample), 10 x 18, 34 x 66 (17 x 33 and 9 x 17), 130 x 94 (33 x 24, 17 x 12)
PICTURES = {
    "rgb192": [(1, (1, 13)), (1, (10, 17)), (1, (10, 18)), (1, (5, 7)), (1, (37, 100)), (2, (65, 18)), (2, (5, 7)), (2, (13, 1)),
               (3, (5, 7)), (3, (33, 257))],
    "yuv420_8b": [(1, (34, 66)), (1, (2, 2)), (2, (34, 66)), (2, (130, 94)), (3, (10, 18))],
    "yuv420_10b": [(1, (10, 18)), (2, (34, 66)), (3, (130, 94))],
    "yuv444_10b": [(1, (37, 100)), (2, (33, 257)), (3, (65, 18))],
}
# the equal-size control (lo = 0: d_out == d_syn_out, the fused epilogue writes the planes), in the donor's own mode
CONTROLS = [("rgb192", (5, 7)), ("rgb192", (37, 100)), ("yuv420_8b", (34, 66)), ("yuv420_10b", (10, 18)), ("yuv444_10b", (65, 18))]
# common randomness: odd sizes at every level, a crop behind every x2 step, levels where one axis stays at 1, lone 1 x 1 levels
CR_SIZES = [(1, 13), (13, 1), (5, 11), (7, 9), (33, 65), (63, 130)]
CR_REFUSED = (1, (10, 17))  # lo = 1: the noise planes have the dense grid's size, not the picture's - refused by both decoders
VIDEOS = [(name, size) for name in ("vid3_hop", "vid3_mop") for size in ((34, 66), (130, 94), (18, 22))]
# one picture per mode that also runs alone in a batch and through add_latents
ALONE = {"nearest": ("rgb192", 1, (37, 100)), "bilinear": ("yuv420_8b", 2, (130, 94)), "bicubic": ("yuv444_10b", 2, (33, 257))}
# derived cases other test files take by name (test_distortion_deltas.py): non-integer scales on both axes
# (19 x 50 -> 37 x 99 and 10 x 25 -> 37 x 99)
NAMED = {"rgb192_37x99_nearest": ("rgb192", 1, "nearest", (37, 99)), "rgb192_37x99_bicubic": ("rgb192", 2, "bicubic", (37, 99))}

# label = "<fixture> <h>x<w> lo=<lo> <mode>"; .levels / .c / .cr / .picture / .label are what float_matrix.describe reads
Case = namedtuple("Case", "label donor lo mode size dense levels c cr picture bitdepth frame_data_type triple stream latents arch")

_CASES = None
_VIDEOS = None
_REF = {}
_PLANES = {}
_MADE = {}


def fmt_class(case):
    return {(8, 0): "rgb8", (8, 1): "yuv420_8", (10, 1): "yuv420_10", (10, 2): "yuv444_10"}[(case.bitdepth, case.frame_data_type)]


def _latents(arch, label):
    """float_matrix's seeded Laplace latents; where every grid is too small for its few forced entries to hold both ends of the
    alphabet (1 x 1 grids), the middle grids' first entries take the missing ones."""
    lat = fm._latents(arch, label)
    for v in (-64, 63):
        if not any((a == v).any() for a in lat):
            g = next(g for g in range(1, len(lat)) if lat[g].flat[0] not in (-64, 63))
            lat[g].flat[0] = v
    return lat


def make(load_golden, oracle, name, lo, mode, size):
    """One picture: the donor's header at another size, its finest grid `lo` levels below the picture, final resize `mode`
    (None: the donor's)."""
    from cool_chic_amd import writer

    key = (name, lo, mode, tuple(size))
    if key in _MADE:
        return _MADE[key]
    donor, ints, fh = fm._donor(load_golden, oracle, name, 0)
    span = donor.latent_resolution[1] - donor.latent_resolution[0]
    changes = dict(img_size=tuple(size), latent_resolution=(lo, lo + span))
    if mode is not None:
        changes["final_upsampling_type"] = MODES.index(mode)
    arch = writer.derive_arch(donor, **changes)
    mode = MODES[arch.final_upsampling_type]
    label = f"{name} {size[0]}x{size[1]} lo={lo} {mode}"
    nn = writer.encode_network(arch, writer.adapt_network(donor, ints, arch))  # (also sets the payload size in `arch`)
    lat = _latents(arch, label)
    stream = writer.encode_stream(writer.cc_header_bytes(arch), nn, lat, bitdepth=int(fh.bitdepth), frame_data_type=int(fh.frame_data_type))
    (_fh, (triple,)), = oracle.split_stream(stream)[1]
    g0 = next(g for g in range(arch.n_grids) if not arch.is_hyperlatent[g])
    levels = sum(1 for g in range(arch.n_grids) if not arch.is_hyperlatent[g])
    _MADE[key] = Case(label, name, lo, mode, tuple(size), (int(arch.grid_h[g0]), int(arch.grid_w[g0])), levels, int(arch.out_channels),
                      bool(arch.flag_common_randomness), True, int(fh.bitdepth), int(fh.frame_data_type), triple, stream, lat, arch)
    return _MADE[key]


def named(load_golden, oracle, name):
    return make(load_golden, oracle, *NAMED[name])


def cases(load_golden, oracle):
    """Every picture and common-randomness case that decodes, in the order the batches hold them."""
    global _CASES
    if _CASES is None:
        out = []
        for name, rows in PICTURES.items():
            for mode in MODES:
                out += [make(load_golden, oracle, name, lo, mode, size) for lo, size in rows]
        out += [make(load_golden, oracle, name, 0, None, size) for name, size in CONTROLS]
        out += [make(load_golden, oracle, "cr192", 0, None, size) for size in CR_SIZES]
        _CASES = out
    return _CASES


def refused(load_golden, oracle):
    return make(load_golden, oracle, "cr192", CR_REFUSED[0], None, CR_REFUSED[1])


def alone(load_golden, oracle):
    """{mode: index into cases()}"""
    cs = cases(load_golden, oracle)
    return {m: next(i for i, c in enumerate(cs) if (c.donor, c.lo, c.size, c.mode) == (d, lo, size, m)) for m, (d, lo, size) in ALONE.items()}


def videos(load_golden, oracle):
    """[(label, stream, [(dense, size, mode) of every cool-chic])]: a video fixture re-written at another picture size the way
    test_video_1080p_gop does - every header derived for the size, the fixture's latents tiled."""
    global _VIDEOS
    from cool_chic_amd import writer

    if _VIDEOS is None:
        out = []
        for name, (H, W) in VIDEOS:
            bs, z, _ = load_golden(name)
            vh, frames = oracle.split_stream(bs)
            parts = [writer.video_header_bytes(vh.n_frames, list(vh.intra_pos[:vh.n_intras]), list(vh.p_pos[:vh.n_p_frames]))]
            k, ccs_info = 0, []
            for fh, ccs in frames:
                parts.append(writer.frame_header_bytes(fh.display_index, "IPB"[fh.frame_type], fh.frame_data_type, fh.bitdepth,
                                                       list(fh.index_references[:fh.n_refs]), list(fh.global_flow[:2 * fh.n_refs]),
                                                       fh.warp_filter_size))
                for hdr, nn, _lat in ccs:
                    donor = writer.parse_cc_header(hdr)
                    arch = writer.derive_arch(donor, img_size=(H, W))
                    lat = [z[f"cc{k}.latent{g}"] for g in range(donor.n_grids)]
                    parts.append(writer.encode_coolchic(arch, nn, writer.tile_latents(lat, donor, arch)))
                    g0 = next(g for g in range(arch.n_grids) if not arch.is_hyperlatent[g])
                    ccs_info.append(((int(arch.grid_h[g0]), int(arch.grid_w[g0])), (H, W), MODES[arch.final_upsampling_type]))
                    k += 1
            out.append((f"{name} {H}x{W}", b"".join(parts), ccs_info))
        _VIDEOS = out
    return _VIDEOS


_VIDEO_REF = {}


def video_reference(oracle, label, stream):
    if label not in _VIDEO_REF:
        _VIDEO_REF[label] = oracle.decode_video(stream)
    return _VIDEO_REF[label]


def reference(oracle, case):
    """oracle.decode_coolchic of the case (latent, dense, syn_out, out), once per process; treat as read-only."""
    if case.label not in _REF:
        r = oracle.decode_coolchic(*case.triple)
        _REF[case.label] = {k: r[k] for k in ("n_grids", "latent", "dense", "syn_out", "out")}
    return _REF[case.label]


def reference_planes(oracle, case):
    if case.label not in _PLANES:
        _PLANES[case.label] = oracle.decode_video(case.stream)[0]["planes"]
    return _PLANES[case.label]


def nearest_branch(n_in, n_out):
    return "equal" if n_in == n_out else ("double" if n_out == 2 * n_in else "general")


def axis_facts(n_in, n_out, mode):
    """(a source coordinate below 0 occurs, a tap index is clamped at n_in - 1) on one axis of an interpolated resize, from the
    exact rational coordinate (n_in (2 dst + 1) - n_out) / (2 n_out)."""
    num = n_in * (2 * np.arange(n_out, dtype=np.int64) + 1) - n_out
    i0 = np.floor_divide(num, 2 * n_out)
    return bool((num < 0).any()), bool((i0 + (2 if mode == "bicubic" else 1) > n_in - 1).any())
