"""The tail of the float path (ccd_float.hip: resize_nearest_kernel, resize_interp_kernel, cr_noise_kernel with its bicubic x2
chain, planes_kernel behind a resize) at ragged sizes: final resizes at non-integer scales in the three
modes, every branch of the nearest rule per axis, 4:2:0 chroma means and 16-bit stores over a resized picture, common
randomness at sizes that are odd at every level, videos whose motion cool-chics sit at non-integer scales
(tests/float_tail.py makes the cases).

Two yardsticks.  The CPU oracle, word for word, for everything the device computes.  And, for the oracle itself, references
that do not restate its code (tests/float_tail_ref.py): F.interpolate for the three resize modes (nearest word-exact, the
interpolated modes within a bar measured per case from torch's own float32 against float64), the noise generator in CPython
`math` (word-exact) with the x2 bicubic chain in float64, and the integer-plane chain in torch float32 (exact)."""
import ctypes as C

import numpy as np
import pytest

import float_matrix as fm
import float_tail as ft
import float_tail_ref as ref
from conftest import load_golden

ORA_ERR_VALUE, CCD_ERR_VALUE = -2, -2


def _word_equal(a, b):
    return fm.first_difference(np.ascontiguousarray(a), np.ascontiguousarray(b)) is None


# ---- CPU -------------------------------------------------------------------------------------------------------------
def test_inventory(oracle):
    """The cases are what they claim: every mode x lo x format class behind a resize; per axis each branch of the nearest rule;
    for the interpolated modes both a source coordinate below 0 and a tap index clamped at in - 1; the equal-size controls;
    every case decodes in the oracle to the latents that were encoded and to a finite output that is not constant; the six
    videos decode, with their motion cool-chics at the non-integer scales named in float_tail.py."""
    cases = ft.cases(load_golden, oracle)
    assert len({c.label for c in cases}) == len(cases)
    resized = [c for c in cases if c.dense != c.size]
    assert all(c.lo > 0 and not c.cr for c in resized) and all(c.lo == 0 for c in cases if c.dense == c.size)
    assert {(c.mode, c.lo, ft.fmt_class(c)) for c in resized} == {(m, lo, f) for m in ft.MODES for lo in ft.LOS for f in ft.DONORS}
    assert {ft.fmt_class(c) for c in cases if c.lo == 0 and not c.cr} == set(ft.DONORS)
    assert [c.size for c in cases if c.cr] == ft.CR_SIZES
    for axis in (0, 1):
        assert {ft.nearest_branch(c.dense[axis], c.size[axis]) for c in resized if c.mode == "nearest"} == {"equal", "double", "general"}, axis
    # exactly x2 on rows with the general rule on columns, exactly x2 on both, equal on one axis only
    both = {(ft.nearest_branch(c.dense[0], c.size[0]), ft.nearest_branch(c.dense[1], c.size[1])) for c in resized if c.mode == "nearest"}
    assert {("double", "general"), ("double", "double"), ("equal", "general"), ("general", "general")} <= both
    for mode in ("bilinear", "bicubic"):
        for axis in (0, 1):
            facts = [ft.axis_facts(c.dense[axis], c.size[axis], mode) for c in resized if c.mode == mode]
            assert any(f[0] for f in facts) and any(f[1] for f in facts), (mode, axis)
        # non-integer scales on both axes, and a 1 x 1 grid (every tap clamped)
        assert any(c.size[0] % c.dense[0] and c.size[1] % c.dense[1] for c in resized if c.mode == mode)
        assert any(c.dense == (1, 1) for c in resized if c.mode == mode)
    for c in cases:
        hdr, nn, lat = c.triple
        h, geo = oracle.read_cc_header(hdr)
        assert (h.nn_n_bytes, h.n_bytes_latent) == (len(nn), len(lat)), c.label
        assert (h.img_size[0], h.img_size[1]) == c.size and h.final_upsampling_type == ft.MODES.index(c.mode), c.label
        g0 = next(g for g in range(geo.n_grids) if not geo.is_hyper[g])
        assert (geo.grid_h[g0], geo.grid_w[g0]) == c.dense == tuple(-(-s >> c.lo) for s in c.size), c.label
        r = ft.reference(oracle, c)
        assert r["n_grids"] == len(c.latents), c.label
        for g, a in enumerate(c.latents):
            assert np.array_equal(r["latent"][g], a), f"{c.label}: the oracle decodes other latents in grid {g}"
        assert {int(a.min()) for a in c.latents} >= {-64} and {int(a.max()) for a in c.latents} >= {63}, c.label
        assert r["out"].shape == (3,) + c.size and r["syn_out"].shape == (3,) + c.dense and np.isfinite(r["out"]).all(), c.label
        if c.dense != (1, 1):
            for ch in range(3):
                assert np.unique(r["out"][ch]).size >= 2, f"{c.label}: channel {ch} is constant"
        assert len(ft.reference_planes(oracle, c)) == 3
    al = ft.alone(load_golden, oracle)
    assert sorted(al) == sorted(ft.MODES) and all(cases[i].dense != cases[i].size for i in al.values())
    want = {(34, 66): (9, 17), (130, 94): (33, 24), (18, 22): (5, 6)}
    for label, stream, ccs in ft.videos(load_golden, oracle):
        frames = ft.video_reference(oracle, label, stream)
        assert len(frames) == 3 and len(ccs) == 5, label
        motion = [(d, s) for d, s, m in ccs if d != s]
        assert len(motion) == 2 and all(m == "nearest" for d, s, m in ccs if d != s), label
        assert all(d == want[s] for d, s in motion), (label, motion)
        assert all(np.unique(p).size >= 2 for f in frames for p in f["planes"]), label
    for name in ft.NAMED:
        c = ft.named(load_golden, oracle, name)
        assert c.size[0] % c.dense[0] and c.size[1] % c.dense[1], name


def test_common_randomness_behind_a_resize_is_refused_by_the_oracle(oracle):
    """A common-randomness stream whose dense grid is smaller than the picture: torch.cat of the latent stack with the noise
    planes fails in the reference; the oracle answers ORA_ERR_VALUE (the library: test_..._by_the_library, on the device)."""
    c = ft.refused(load_golden, oracle)
    assert c.cr and c.dense != c.size
    hdr, nn, lat = c.triple
    r = oracle.CCResult()
    rc = oracle.lib().ora_decode_coolchic(hdr, len(hdr), nn, len(nn), lat, len(lat), 0, C.byref(r))
    oracle.lib().ora_cc_result_free(C.byref(r))
    assert rc == ORA_ERR_VALUE


NEAREST_SWEEP_OUT = list(range(1, 700)) + [1079, 1080, 1365, 2047, 2160, 3839, 16383]


def test_nearest_index_rule_against_torch():
    """The nearest rule (equal / exactly x2 / floorf(dst * in/out), min with in - 1) restated in numpy against F.interpolate of an
    arange: input sizes ceil(out / 2^lo), lo = 1 .. 4, output sizes 1 .. 699 and a few video sizes - every index vector."""
    n, bad = 0, []
    for n_out in NEAREST_SWEEP_OUT:
        for lo in (1, 2, 3, 4):
            n_in = -(-n_out >> lo)
            n += 1
            if not np.array_equal(ref.nearest_index(n_in, n_out), ref.nearest_index_torch(n_in, n_out)):
                bad.append((n_in, n_out))
    assert n == 4 * len(NEAREST_SWEEP_OUT) == 2824
    assert not bad, (len(bad), bad[:8])


def test_nearest_reference_against_the_oracle(oracle):
    """syn_out -> out of every nearest case == F.interpolate(mode="nearest"), as words."""
    bad = []
    n = 0
    for c in ft.cases(load_golden, oracle):
        if c.mode == "nearest" and c.dense != c.size:
            r = ft.reference(oracle, c)
            bad.append(fm.describe(c, "-", "oracle out", r["out"], ref.nearest(r["syn_out"], c.size), "F.interpolate(nearest)"))
            n += 1
    assert n >= 21
    bad = [m for m in bad if m]
    assert not bad, "\n".join(bad[:8])


def _interp_check(label, got, x, size, mode, worst):
    want = ref.interp64(x, size, mode)
    bar, measured = ref.interp_bar(x, size, mode, want)
    dev = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{label}: |oracle - f64| {dev:.3g}, torch f32 - f64 {measured:.3g}, bar {bar:.3g}, ratio to the bar {dev / bar:.3f}")
    worst[mode] = max(worst.get(mode, 0.0), dev / bar)
    return None if dev <= bar else f"{label}: {dev:.4g} from the float64 F.interpolate, bar {bar:.4g} (torch float32: {measured:.4g})"


def test_interpolated_reference_against_the_oracle(oracle):
    """syn_out -> out of every bilinear / bicubic case, and ora_debug_resize on seeded N(0, 1) planes at the same size pairs,
    against F.interpolate(align_corners=False) in float64, within the measured bar of float_tail_ref.py."""
    bad, worst, pairs = [], {}, {}
    for c in ft.cases(load_golden, oracle):
        if c.mode != "nearest" and c.dense != c.size:
            r = ft.reference(oracle, c)
            bad.append(_interp_check(c.label, r["out"], r["syn_out"], c.size, c.mode, worst))
            pairs[(c.dense, c.size, c.mode)] = True
    rng = np.random.default_rng(20251018)
    for dense, size, mode in pairs:
        x = rng.standard_normal((3,) + dense).astype(np.float32)
        got = oracle.debug_resize(x, size, mode == "bicubic")
        bad.append(_interp_check(f"N(0, 1) {dense} -> {size} {mode}", got, x, size, mode, worst))
    print("largest ratio to the bar:", {k: round(v, 3) for k, v in worst.items()})
    assert len(pairs) >= 30
    bad = [m for m in bad if m]
    assert not bad, "\n".join(bad[:8])


def _level_sizes(c):
    a = c.arch
    return [(int(a.grid_h[g]), int(a.grid_w[g])) for g in range(a.n_grids) if not a.is_hyperlatent[g]]


_NOISE = {}


def _noise(n):
    """The first n samples in CPython `math`, made once for the largest n asked (the tests ask for the largest first)."""
    if "s" not in _NOISE or _NOISE["s"].size < n:
        _NOISE["s"] = ref.noise_samples(n)
    return _NOISE["s"][:n]


def test_noise_reference_against_the_oracle(oracle):
    """400 000 samples of the oracle's generator == the Park-Miller / Box-Muller loop in CPython `math`, as words; the dense
    channels [L, 2L) of the six common-randomness cases against the x2 bicubic chain in float64, within the measured bar."""
    n = 400000
    assert _word_equal(oracle.debug_cr_noise(n), _noise(n))
    bad, worst = [], 0.0
    for c in ft.cases(load_golden, oracle):
        if c.cr:
            L = c.levels
            got = ft.reference(oracle, c)["dense"][L:2 * L]
            want, bar, measured = ref.noise_chain(_level_sizes(c), _noise(n))
            dev = float(np.abs(got.astype(np.float64) - want).max())
            print(f"{c.label}: |oracle - f64| {dev:.3g}, torch f32 - f64 {measured:.3g}, bar {bar:.3g}, ratio to the bar {dev / bar:.3f}")
            worst = max(worst, dev / bar)
            assert _word_equal(got[0], _noise(c.size[0] * c.size[1]).reshape(c.size)), c.label  # the finest plane is the samples
            if dev > bar:
                bad.append(f"{c.label}: {dev:.4g} from the float64 chain, bar {bar:.4g}")
    print("largest ratio to the bar:", round(worst, 3))
    assert not bad, "\n".join(bad)


def test_plane_reference_against_the_oracle(oracle):
    """Integer planes of oracle.decode_video == the literal torch float32 chain over the oracle's `out`: every sample of every
    case (8-bit RGB, 4:2:0 at 8 and 10 bits, 10-bit 4:4:4), resized or not."""
    bad, n, inside = [], 0, 0
    for c in ft.cases(load_golden, oracle):
        want = ref.planes(ft.reference(oracle, c)["out"], c.bitdepth, c.frame_data_type)
        for p, (a, w) in enumerate(zip(ft.reference_planes(oracle, c), want)):
            bad.append(fm.describe(c, "-", f"oracle plane {p}", a, w, "torch float32 chain"))
            n += a.size
            inside += int(((a > 0) & (a < (1 << c.bitdepth) - 1)).sum())
    print(f"{n} samples, {inside} of them strictly inside the range")
    assert inside > n // 4  # the comparison is not one of saturated samples
    bad = [m for m in bad if m]
    assert not bad, "\n".join(bad[:8])


FOOTPRINT_SIZES = [(5, 7), (37, 100), (65, 18), (33, 257), (127, 191)]


def test_footprint_by_impulse_in_the_oracle(oracle):
    """ccd_latent_footprint (derived per mode from the final-resize tap rule, ccd_dsens_api.cpp) behind a resize: rgb192 at five
    sizes x lo 1 .. 3 x three modes; in every latent grid one latent flipped between the ends of the alphabet at the four corners,
    the centre and three seeded positions, re-encoded and decoded by the oracle: no output word outside the box changes, and on
    every side the box (clipped to the picture, as _box_of gives it) is tight (slack 0) for some flip.  Where the picture does not
    clip it the box keeps the half source sample it adds for the float32 coordinate: that slack is printed."""
    from test_distortion_deltas import _box_of

    from cool_chic_amd import writer
    from cool_chic_amd.dsens import latent_footprint

    def decode(arch, nn, lat):
        blob = writer.encode_coolchic(arch, nn, lat)
        h = writer.parse_cc_header(blob)
        a, b = h.n_bytes_header, h.n_bytes_header + h.nn_n_bytes
        return oracle.decode_coolchic(blob[:a], blob[a:b], blob[b:])["out"].view(np.uint32)

    rng = np.random.default_rng(20251019)
    n_flips, n_free, slack, inner = 0, 0, [None] * 4, [None] * 4
    for size in FOOTPRINT_SIZES:
        for lo in ft.LOS:
            for mode in ft.MODES:
                c = ft.make(load_golden, oracle, "rgb192", lo, mode, size)
                arch, nn = c.arch, c.triple[1]
                H, W = size
                base = decode(arch, nn, c.latents)
                for g in range(arch.n_grids):
                    if arch.is_hyperlatent[g]:
                        continue
                    h, w = c.latents[g].shape
                    pos = {(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2)}
                    pos |= {(int(rng.integers(h)), int(rng.integers(w))) for _ in range(3)}
                    box = latent_footprint(arch, g)
                    for y, x in sorted(pos):
                        l2 = list(c.latents)
                        l2[g] = c.latents[g].copy()
                        l2[g][y, x] = 63 if l2[g][y, x] < 0 else -64
                        diff = (decode(arch, nn, l2) != base).any(axis=0)
                        n_flips += 1
                        y0, x0, y1, x1 = _box_of(arch, g, y, x, box)
                        rows, cols = np.flatnonzero(diff.any(axis=1)), np.flatnonzero(diff.any(axis=0))
                        assert rows.size, (c.label, g, y, x)
                        found = (rows[0], cols[0], rows[-1], cols[-1])
                        assert found[0] >= y0 and found[1] >= x0 and found[2] <= y1 and found[3] <= x1, \
                            (c.label, g, y, x, "changed", found, "box", (y0, x0, y1, x1))
                        # slack of the (clipped) box per side; apart, on the sides where the picture does not clip it
                        sides = [(y0 > 0, found[0] - y0), (x0 > 0, found[1] - x0), (y1 < H - 1, y1 - found[2]), (x1 < W - 1, x1 - found[3])]
                        for k, (free, s) in enumerate(sides):
                            slack[k] = int(s) if slack[k] is None else min(slack[k], int(s))
                            if free:
                                inner[k] = int(s) if inner[k] is None else min(inner[k], int(s))
                                n_free += 1
    print(f"{n_flips} flips, smallest slack (top, left, bottom, right) {slack}; on the {n_free} sides the picture does not clip {inner}")
    assert n_flips > 1200 and n_free > 1200
    assert slack == [0, 0, 0, 0]


# ---- GPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cool_chic_amd import DecodeBatch, _lib

    _lib.lib()
    return DecodeBatch


def _read(b, slot, case):
    k = b.slot_kernels(slot)
    return {"status": b.slot_status(slot), "kernels": k, "latent": [b.latent(slot, g) for g in range(len(case.latents))],
            "output": b.output(slot), "dense": None if k & 4 else b.dense(slot), "planes": b.planes(slot)}


_BATCH = {}


def _decoded(gpu, oracle, form):
    """ALL picture and common-randomness cases in ONE batch with CCD_OPT_FUSED_DEC = form.  Once per process; a batch that failed
    is not run again."""
    if form not in _BATCH:
        cases = ft.cases(load_golden, oracle)
        try:
            b = gpu(0, fused_dec=form)
            try:
                for c in cases:
                    b.add(*c.triple, c.bitdepth, c.frame_data_type)
                b.run()
                b.wait()
                _BATCH[form] = [_read(b, i, c) for i, c in enumerate(cases)]
            finally:
                b.close()
        except Exception as e:
            _BATCH[form] = e
    if isinstance(_BATCH[form], Exception):
        raise _BATCH[form]
    return _BATCH[form]


def _expected_fused(case, form):
    """(bit 2: the fused float kernel, bit 6: its form behind the pyramid launch) a slot must report; a final resize does not
    change which kernel computes the synthesis output."""
    if form == 0 or (case.cr and form == 1):  # the one-launch form has no common-randomness instantiation
        return False, False
    return True, form == 2


@pytest.mark.gpu
@pytest.mark.parametrize("form", [2, 1, 0])
def test_all_pictures_in_one_batch(gpu, oracle, form):
    """`output` == the oracle's `out`, every integer plane == oracle.decode_video's, as words; unfused (form 0, and common
    randomness in form 1) also `dense` == the oracle's, noise channels included, and the finest noise plane == the CPython words."""
    cases = ft.cases(load_golden, oracle)
    got = _decoded(gpu, oracle, form)
    bad, n_noise = [], 0
    for c, r in zip(cases, got):
        want = ft.reference(oracle, c)
        k = r["kernels"]
        if r["status"] != 0:
            bad.append(f"{c.label} fused_dec={form}: slot status {r['status']}")
        fused, pre = _expected_fused(c, form)
        if (bool(k & 4), bool(k & 64)) != (fused, pre) or k & 128 or k & 256 or (form == 0 and k & 8):
            bad.append(f"{c.label} fused_dec={form}: slot_kernels {k:#x}, expected bit 2 {fused}, bit 6 {pre}, bits 3 (unfused), 7 and 8 clear")
        for g, a in enumerate(c.latents):
            if not np.array_equal(r["latent"][g], a):
                bad.append(f"{c.label} fused_dec={form}: latent grid {g} differs from what was encoded")
        bad.append(fm.describe(c, form, "output behind the final resize", r["output"], want["out"]))
        if not fused:
            assert r["dense"] is not None
            bad.append(fm.describe(c, form, "dense stack", r["dense"], want["dense"]))
            if c.cr:
                samples = _noise(c.size[0] * c.size[1]).reshape(c.size)
                bad.append(fm.describe(c, form, "finest noise plane", r["dense"][c.levels], samples, "CPython math"))
                n_noise += 1
        for p, (a, w) in enumerate(zip(r["planes"], ft.reference_planes(oracle, c))):
            assert a.dtype == (np.uint8 if c.bitdepth == 8 else np.uint16), c.label
            bad.append(fm.describe(c, form, f"integer plane {p}", a.astype(np.uint16), w))
    if form != 2:
        assert n_noise == len(ft.CR_SIZES)
    bad = [m for m in bad if m]
    assert not bad, f"{len(bad)} failures, the first of them:\n" + "\n".join(bad[:12])


@pytest.mark.gpu
def test_common_randomness_behind_a_resize_is_refused_by_the_library(gpu, oracle):
    """ccd_batch_add answers CCD_ERR_VALUE (ccd_batch_plan.cpp: s.cr && p.need_resize); the batch stays usable."""
    from cool_chic_amd._lib import CcdError

    c = ft.refused(load_golden, oracle)
    ok = ft.cases(load_golden, oracle)[-1]
    b = gpu(0)
    try:
        with pytest.raises(CcdError) as e:
            b.add(*c.triple, c.bitdepth, c.frame_data_type)
        assert e.value.code == CCD_ERR_VALUE
        b.add(*ok.triple, ok.bitdepth, ok.frame_data_type)
        b.run()
        b.wait()
        assert b.slot_status(0) == 0
    finally:
        b.close()


def _same_as_big_batch(c, r, want, how):
    bad = [fm.describe(c, how, "output", r["output"], want["output"], "in the big batch")]
    bad += [fm.describe(c, how, f"integer plane {p}", a, w, "in the big batch") for p, (a, w) in enumerate(zip(r["planes"], want["planes"]))]
    bad = [m for m in bad if m]
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ft.MODES)
def test_alone_equals_the_big_batch(gpu, oracle, mode):
    """One resized picture of the mode ALONE in a batch (default form): with one entropy launch the resize and planes launches
    follow it on the caller's stream (the other branch of launch_entropy_groups / tail_keyed).  Same words as in the big batch."""
    cases = ft.cases(load_golden, oracle)
    i = ft.alone(load_golden, oracle)[mode]
    c, want = cases[i], _decoded(gpu, oracle, 2)[i]
    b = gpu(0, fused_dec=2)
    try:
        b.add(*c.triple, c.bitdepth, c.frame_data_type)
        b.run()
        b.wait()
        r = _read(b, 0, c)
    finally:
        b.close()
    assert r["status"] == 0 and r["kernels"] == want["kernels"] and r["kernels"] & 68 == 68, (c.label, r["status"], r["kernels"], want["kernels"])
    _same_as_big_batch(c, r, want, "2 alone")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ft.MODES)
def test_given_latents_equal_the_coded_slot(gpu, oracle, mode):
    """The same picture through ccd_batch_add_latents (no entropy launch: bit 8): the words of the coded slot."""
    cases = ft.cases(load_golden, oracle)
    i = ft.alone(load_golden, oracle)[mode]
    c, want = cases[i], _decoded(gpu, oracle, 2)[i]
    b = gpu(0, fused_dec=2)
    try:
        b.add_latents(c.arch, c.triple[1], c.latents, c.bitdepth, c.frame_data_type)
        b.run()
        b.wait()
        r = _read(b, 0, c)
    finally:
        b.close()
    assert r["status"] == 0 and r["kernels"] & 256 and r["kernels"] & 68 == 68, (c.label, r["status"], r["kernels"])
    _same_as_big_batch(c, r, want, "2 given latents")


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(ft.VIDEOS)))
def test_video_with_motion_at_a_ragged_scale(gpu, oracle, k):
    """ccd_decode_video: the motion cool-chics' nearest resize at 9 x 17 -> 34 x 66, 33 x 24 -> 130 x 94 and 5 x 6 -> 18 x 22
    feeds the warp; every plane of every frame == oracle.decode_video."""
    from cool_chic_amd._lib import Video, check, lib

    label, stream, _ = ft.videos(load_golden, oracle)[k]
    want = ft.video_reference(oracle, label, stream)
    v = Video()
    check(lib().ccd_decode_video(stream, len(stream), 0, C.byref(v)), "ccd_decode_video")
    try:
        assert v.n_frames == len(want)
        for i in range(v.n_frames):
            f = v.frames[i]
            for p, shape in enumerate([(f.h, f.w), (f.ch, f.cw), (f.ch, f.cw)]):
                assert shape == want[i]["planes"][p].shape, (label, i, p)
                got = np.ctypeslib.as_array(f.plane[p], shape=shape)
                d = fm.first_difference(got, want[i]["planes"][p])
                assert d is None, f"{label} frame {i} plane {p}: {d[1]} samples differ, first at (row, column) = {d[0]}"
    finally:
        lib().ccd_video_free(C.byref(v))
