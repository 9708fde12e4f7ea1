"""Cool-chics that reach EVERY instantiation of the fused float kernel (ccd_fused_kernel.inc::decode_fused_kernel<CIN, C, MODE, NZ>,
DESIGN.md section 4.2): 5 .. 9 latent levels x 2 .. 4 .. 5 output channels, common randomness (NZ = CIN) at every level count, at
the smallest dense-grid sizes that reach each mechanism of the tile walk.  Manufactured with this repo's writer from the trained
networks of reference-encoded fixtures (grown to the level count with writer.adapt_network) and seeded latents; the yardstick
is the CPU oracle.  Shared by the CPU inventory test and the GPU parity tests of tests/test_float_matrix.py; every stream and
every oracle result is made once per process."""
import zlib
from collections import namedtuple

import numpy as np

LEVELS = (5, 6, 7, 8, 9)
CHANNELS = (2, 3, 4, 5)

# (fixture, cool-chic index in stream order = oracle.split_stream's order = z["cc{k}.nn_ints"]'s numbering, note)
DONORS = [
    ("vid3_hop", 2, "motion, latent levels 2 .. : the dense grid is a quarter of the picture, a final resize follows"),
    ("rgb192", 0, "lop, 3 synthesis layers"),
    ("vid3_hop", 0, "vhop: 64 hidden units, 4 layers"),
    ("vid3_hop", 1, "residue hop: 48 hidden"),
    ("vid3_vlop", 1, "residue vlop: 8 hidden"),
    ("vid3_hop", 3, "residue hop (B frame): 48 hidden"),
    ("vid5", 3, "residue lop: 16 hidden"),
    ("cr192", 0, "common randomness: NZ = CIN"),
]
EXPECTED_C = {("vid3_hop", 2): 2, ("rgb192", 0): 3, ("vid3_hop", 0): 3, ("vid3_hop", 1): 4, ("vid3_vlop", 1): 4, ("vid3_hop", 3): 5,
              ("vid5", 3): 5, ("cr192", 0): 3}
# dense-grid sizes (h, w) every donor runs at every level count.  The kernel's tile is 64 columns x 32 rows, a workgroup takes a
# run of up to 8 tiles: one row and one column past a tile (four tiles, three of them almost empty; with 9 levels the coarsest
# grids are 1 x 2 and 2 x 3: every footprint is clamped) / smaller than every halo and margin / exact multiples of the tile
SIZES = [(33, 65), (7, 9), (64, 128)]
# more than one run of 8 tiles (24 tiles: the per-run parameter staging happens more than once in a frame): one donor per C (and
# the common-randomness one), fewest and most levels
LARGE = (97, 321)
LARGE_DONORS = [("vid3_hop", 2), ("rgb192", 0), ("vid3_hop", 1), ("vid5", 3), ("cr192", 0)]
LARGE_LEVELS = (5, 9)
# the integer epilogue at level counts other than 7: (fixture, levels, picture size)
FORMATS = [("yuv420_8b", 5, (34, 66)), ("yuv420_8b", 9, (34, 66)),    # the per-quad chroma mean next to a tile border
           ("yuv444_10b", 6, (33, 65)), ("yuv444_10b", 8, (33, 65))]  # the 16-bit plane stores
# one case per (levels, C) at 33 x 65 that also runs alone in a batch
ALONE_DONORS = {2: ("vid3_hop", 2), 3: ("rgb192", 0), 4: ("vid3_hop", 1), 5: ("vid3_hop", 3)}

# label = "<fixture>.cc<k> n=<levels> dense=<h>x<w>"; picture: a C = 3 cool-chic framed as a one-frame stream (integer planes
# exist: `stream`, bitdepth, frame_data_type); the others go into a batch with bitdepth 0 (float output only)
Case = namedtuple("Case", "label donor cc levels dense c cr picture bitdepth frame_data_type triple stream latents arch")

_DONOR = {}
_CASES = None
_REF = {}
_PLANES = {}


def _donor(load_golden, oracle, name, k):
    """(parsed header, network integers, frame header) of cool-chic k of a fixture."""
    from cool_chic_amd import writer

    if (name, k) not in _DONOR:
        bs, z, _ = load_golden(name)
        ccs = [(fh, cc) for fh, ccs_ in oracle.split_stream(bs)[1] for cc in ccs_]
        fh, (hdr, _nn, _lat) = ccs[k]
        _DONOR[(name, k)] = (writer.parse_cc_header(hdr), np.asarray(z[f"cc{k}.nn_ints"]), fh)
    return _DONOR[(name, k)]


def _latents(arch, label):
    """Seeded Laplace latents (as test_ragged_picture_sizes draws them) with a few entries at the ends of the symbol range,
    -64 and 63, in the finest and in the coarsest grid (of the synthesis' pyramid, and the last grid of the stream)."""
    rng = np.random.default_rng(zlib.crc32(label.encode()))
    lat = [np.clip(np.rint(rng.laplace(0.0, 1.2, size=(arch.grid_h[g], arch.grid_w[g]))), -20, 20).astype(np.int8)
           for g in range(arch.n_grids)]
    pyramid = [g for g in range(arch.n_grids) if not arch.is_hyperlatent[g]]
    for g in sorted({pyramid[0], pyramid[-1], arch.n_grids - 1}):
        flat = lat[g].reshape(-1)
        pos = rng.choice(flat.size, size=min(4, flat.size), replace=False)
        flat[pos] = np.array([-64, 63, 63, -64], np.int8)[: pos.size]
    return lat


def _make(load_golden, oracle, name, k, n, dense, as_picture):
    from cool_chic_amd import writer

    donor, ints, fh = _donor(load_golden, oracle, name, k)
    lo = donor.latent_resolution[0]
    hi = lo + n - 1
    changes = dict(img_size=(dense[0] << lo, dense[1] << lo), latent_resolution=(lo, hi), n_latent_grids=n)
    if donor.flag_hyperlatent:
        changes["hyperlatent_resolution"] = (min(4, hi), hi)
        changes["n_latent_grids"] = n + hi - min(4, hi) + 1
    arch = writer.derive_arch(donor, **changes)
    assert (arch.grid_h[0], arch.grid_w[0]) == tuple(dense), (name, k, n, dense)
    label = f"{name}.cc{k} n={n} dense={dense[0]}x{dense[1]}"
    nn = writer.encode_network(arch, writer.adapt_network(donor, ints, arch))  # (also sets the payload size in `arch`)
    lat = _latents(arch, label)
    c, cr = int(arch.out_channels), bool(arch.flag_common_randomness)
    if as_picture is not None:
        bitdepth, fdt = as_picture
        stream = writer.encode_stream(writer.cc_header_bytes(arch), nn, lat, bitdepth=bitdepth, frame_data_type=fdt)
        (_fh, (triple,)), = oracle.split_stream(stream)[1]
    else:
        bitdepth, fdt, stream = 0, int(fh.frame_data_type), None
        blob = writer.encode_coolchic(arch, nn, lat)
        h = writer.parse_cc_header(blob)
        a, b = h.n_bytes_header, h.n_bytes_header + h.nn_n_bytes
        assert len(blob) == b + h.n_bytes_latent, label
        triple = (blob[:a], blob[a:b], blob[b:])
    return Case(label, name, k, n, tuple(dense), c, cr, as_picture is not None, bitdepth, fdt, triple, stream, lat, arch)


def cases(load_golden, oracle):
    """Every case, in the order the batches hold them."""
    global _CASES
    if _CASES is None:
        out = []
        for name, k, _note in DONORS:
            donor, _, fh = _donor(load_golden, oracle, name, k)
            # a three-channel cool-chic is a picture: rgb192 / cr192 in their own format; the I frame of vid3_hop is 4:2:0 in its
            # fixture, which the odd sizes here cannot be, and goes in as 8-bit RGB (4:2:0: the yuv420_8b cases below)
            pic = None
            if donor.out_channels == 3:
                pic = (int(fh.bitdepth), int(fh.frame_data_type)) if fh.frame_data_type != 1 else (8, 0)
            for n in LEVELS:
                for dense in SIZES:
                    out.append(_make(load_golden, oracle, name, k, n, dense, pic))
                if (name, k) in LARGE_DONORS and n in LARGE_LEVELS:
                    out.append(_make(load_golden, oracle, name, k, n, LARGE, pic))
        for name, n, size in FORMATS:
            _, _, fh = _donor(load_golden, oracle, name, 0)
            out.append(_make(load_golden, oracle, name, 0, n, size, (int(fh.bitdepth), int(fh.frame_data_type))))
        _CASES = out
    return _CASES


def reference(oracle, case):
    """oracle.decode_coolchic of the case (latent, dense, out), once per process; treat as read-only."""
    if case.label not in _REF:
        r = oracle.decode_coolchic(*case.triple)
        _REF[case.label] = {k: r[k] for k in ("n_grids", "latent", "dense", "out")}
    return _REF[case.label]


def reference_planes(oracle, case):
    """Integer planes of a picture case: oracle.decode_video of its one-frame stream, once per process."""
    if case.label not in _PLANES:
        _PLANES[case.label] = oracle.decode_video(case.stream)[0]["planes"]
    return _PLANES[case.label]


def first_difference(got, want):
    """None when the two arrays hold the same words (float32 compared as uint32: no tolerance, -0.0 != 0.0), else
    (index of the first differing element in C order, number of differing elements)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        raise AssertionError(f"shape / type {got.shape} {got.dtype} against {want.shape} {want.dtype}")
    view = {1: np.uint8, 2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    bad = got.view(view) != want.view(view)
    if not bad.any():
        return None
    return tuple(int(i) for i in np.unravel_index(int(np.argmax(bad)), bad.shape)), int(bad.sum())


def describe(case, form, what, got, want, yardstick="oracle"):
    """None, or the failure message: donor, level count, size, form, what was compared, channel and first differing (row, column)."""
    d = first_difference(got, want)
    if d is None:
        return None
    idx, n = d
    where = f"channel {idx[0]}, first differing (row, column) = ({idx[1]}, {idx[2]})" if len(idx) == 3 else f"first differing (row, column) = {idx}"
    g, w = np.asarray(got)[idx], np.asarray(want)[idx]
    return f"{case.label} C={case.c}{' common randomness' if case.cr else ''} fused_dec={form}: {what}: {n} of {np.asarray(want).size} words differ; {where}: got {g!r}, {yardstick} {w!r}"
