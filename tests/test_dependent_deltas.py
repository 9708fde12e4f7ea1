"""Distortion deltas through the frames that predict from a moved one (ccd_dsens_add_dependent, DistortionDeltas.add_dependent;
DESIGN.md section 4.16): for every latent of a frame R the exact change of the squared error of the P / B frames that read R's
planes as a reference, if that latent were v - 1 or v + 1.

The reference is brute force from public calls (tests/dependent_cases.py): one latent moved on the host, R decoded, every dependent
through ccd_inter_reconstruct against the moved planes, QualityMeter, minus the base.  Everything is compared as integers, with no
tolerance."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

ERR_VALUE, ERR_ARG = -2, -7
SENTINEL = -2 ** 63
ENTRY_POINTS = ["ccd_dsens_add_dependent", "ccd_dsens_slot_dep_map", "ccd_dsens_slot_dep_conflicts", "ccd_latent_probe_stride_margin",
                "ccd_debug_lattice_stride", "ccd_debug_lattice_hit"]


# ---- CPU -------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    from cool_chic_amd import _lib

    with open(os.path.join(ROOT, "include", "ccd.h")) as f:
        header = f.read()
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert name + "(" in header, name
        assert name in _lib.SIGNATURES, name
        assert getattr(L, name) is not None
    assert "} ccd_dsens_dependent;" in header and hasattr(_lib, "DsensDependent")
    import cool_chic_amd
    from cool_chic_amd import dsens, rd

    assert all(hasattr(cool_chic_amd.DistortionDeltas, m) for m in ("add_dependent", "dep_delta_map", "dep_conflicts"))
    assert all(hasattr(rd.RdEvaluator, m) for m in ("add_dependent", "dependent_delta_map"))
    assert "margin" in dsens.probe_stride.__code__.co_varnames and "dependents" in rd.RdEvaluator.cost_delta_map.__code__.co_varnames


def test_argument_errors_without_a_device():
    """Every refusal of ccd_dsens_add_dependent comes before the handle's slots or the device are looked at: the handle is 1 KiB
    of zeros (it holds no slot, so a call that passes every other check ends at the bad slot)."""
    from cool_chic_amd._lib import DsensDependent, lib

    L = lib()
    handle = C.create_string_buffer(1024)
    d = C.cast(handle, C.c_void_p)
    buf = np.zeros(16, np.float32)
    a = buf.ctypes.data

    def add(handle=d, slot=0, dep="default", frame_type=1, which=0, residue=a, motion=a, other=(0, 0, 0), src=(a, a, a), taps=8):
        if dep == "default":
            dep = DsensDependent(frame_type=frame_type, which=which, residue=residue or None, motion=motion or None,
                                 other_ref=(C.c_void_p * 3)(*[p or None for p in other]), src=(C.c_void_p * 3)(*[p or None for p in src]),
                                 global_flow=(C.c_int32 * 4)(0, 0, 0, 0), warp_filter_size=taps)
        return L.ccd_dsens_add_dependent(handle, slot, C.byref(dep) if dep is not None else None)

    assert add(handle=None) == ERR_ARG and add(dep=None) == ERR_ARG
    assert add(residue=0) == ERR_ARG and add(motion=0) == ERR_ARG
    for p in range(3):
        planes = [a, a, a]
        planes[p] = 0
        assert add(src=tuple(planes)) == ERR_ARG
        assert add(frame_type=2, other=tuple(planes)) == ERR_ARG   # a B frame needs the planes of its other reference
    for frame_type in (0, 3, -1):
        assert add(frame_type=frame_type) == ERR_ARG
    for which in (-1, 2):
        assert add(which=which) == ERR_ARG and add(frame_type=2, other=(a, a, a), which=which) == ERR_ARG
    assert add(which=1) == ERR_ARG                                  # a P frame has one reference
    for slot in (0, -1, 1, 1 << 20):                                # the zero handle holds no slot
        assert add(slot=slot) == ERR_ARG and add(frame_type=2, which=1, other=(a, a, a), slot=slot) == ERR_ARG
    pending = C.create_string_buffer(1024)                          # a run in flight: whatever the handle holds says so
    pending.raw = b"\x01" * 1024
    assert add(handle=C.cast(pending, C.c_void_p)) == ERR_ARG
    for taps in (0, 1, 3, 7, 18, -2):
        assert add(taps=taps) == ERR_VALUE, taps
    assert bytes(handle) == bytes(1024) and bytes(pending) == b"\x01" * 1024
    dev = C.c_void_p()
    assert L.ccd_dsens_slot_dep_map(None, 0, 0, C.byref(dev)) == ERR_ARG and L.ccd_dsens_slot_dep_map(d, 0, 0, None) == ERR_ARG
    assert L.ccd_dsens_slot_dep_map(d, 0, 0, C.byref(dev)) == ERR_ARG and not dev.value
    assert L.ccd_dsens_slot_dep_conflicts(None, 0, 0) == ERR_ARG and L.ccd_dsens_slot_dep_conflicts(d, 0, 0) == ERR_ARG


def _axes(arch, g):
    """Per axis (n, N, lo, hi, num, den) of latent grid g as include/ccd.h states the footprint."""
    from cool_chic_amd.dsens import latent_footprint

    lat = [k for k in range(arch.n_grids) if not arch.is_hyperlatent[k]]
    pitch = 1 << lat.index(g)
    top, left, bottom, right = latent_footprint(arch, g)
    return [(int(arch.grid_h[g]), int(arch.img_size[0]), top, bottom, pitch * int(arch.img_size[0]), int(arch.grid_h[lat[0]])),
            (int(arch.grid_w[g]), int(arch.img_size[1]), left, right, pitch * int(arch.img_size[1]), int(arch.grid_w[lat[0]]))]


def _regions(axis, even):
    n, N, lo, hi, num, den = axis
    s = (np.arange(n, dtype=np.int64) * num) // den
    a, b = np.maximum(s + lo, 0), np.minimum(s + hi, N - 1)
    if even:
        a, b = a & ~1, b | 1
    return a, b


def _stride_ref(axis, even, margin):
    n = axis[0]
    a, b = _regions(axis, even)
    for S in range(1, n):
        if np.all(a[S:] - b[:-S] - 1 >= margin):
            return S
    return max(n, 1)


def _lattice_arches():
    import arm_layouts
    import inter_cases as ic
    from test_distortion_deltas import _arch

    out = [(name, _arch(name)[0]) for name in ("odd18x65", "rgb192", "bicubic190", "yuv420_8b", "odd100x37", "rgb192_37x99_bicubic")]
    out += [(f"vid3_ldp[1].{i}", cc[0]) for i, cc in enumerate(ic.parse_video("vid3_ldp")[1][1])]
    out += [(c.name, c.arch) for c in arm_layouts.cases() if tuple(c.img_size) in ((18, 65), (37, 100)) and c.kind in ("arm", "placement")][:6]
    return out


def test_lattice_geometry_against_enumeration():
    """ccd_debug_lattice_stride / ccd_debug_lattice_hit (csrc/ccd_lattice.hpp on the host) against a numpy enumeration of the
    regions: fixtures' and ragged arches, margins 0, 1, 7, 10, with and without the even widening; at margin 0 without widening
    the stride is ccd_latent_probe_stride's for rgb."""
    from cool_chic_amd._lib import lib
    from cool_chic_amd.dsens import probe_stride

    L = lib()
    rng = np.random.default_rng(16)
    n_hits = {-2: 0, -1: 0, 1: 0}
    arches = _lattice_arches()
    assert len(arches) >= 10
    for name, arch in arches:
        for g in range(arch.n_grids):
            if arch.is_hyperlatent[g]:
                assert probe_stride(arch, g, 0, margin=7) == 0
                continue
            axes = _axes(arch, g)
            for even in (0, 1):
                per_margin = {}
                for margin in (0, 1, 7, 10):
                    strides = []
                    for axis in axes:
                        want = _stride_ref(axis, even, margin)
                        got = L.ccd_debug_lattice_stride(*axis, even, margin)
                        assert got == want, (name, g, axis, even, margin, got, want)
                        strides.append(want)
                    per_margin[margin] = max(strides)
                    assert probe_stride(arch, g, 1 if even else 0, margin=margin) == max(strides), (name, g, even, margin)
                    assert even or probe_stride(arch, g, 2, margin=margin) == max(strides)
                if not even:
                    assert per_margin[0] == L.ccd_latent_probe_stride(C.byref(arch), g, 0), (name, g)
                assert per_margin[0] <= per_margin[1] <= per_margin[7] <= per_margin[10]
                for axis in axes:
                    n, N = axis[0], axis[1]
                    ra, rb = _regions(axis, even)
                    for S in sorted({1, 2, per_margin[0], per_margin[7], n}):
                        for phase in sorted({0, min(S, n) - 1, int(rng.integers(min(S, n)))}):
                            members = np.arange(phase, n, S)
                            for _ in range(12):
                                a = int(rng.integers(0, N))
                                b = min(N - 1 + (N & even), a + int(rng.integers(0, 12)))
                                hit = members[(ra[members] <= b) & (rb[members] >= a)]
                                want = -1 if len(hit) == 0 else (int(hit[0]) if len(hit) == 1 else -2)
                                first, count = C.c_int32(-5), C.c_int32(-5)
                                got = L.ccd_debug_lattice_hit(*axis, even, S, phase, a, b, C.byref(first), C.byref(count))
                                assert got == want, (name, g, axis, even, S, phase, a, b, got, want)
                                assert count.value == len(hit) and first.value == (int(hit[0]) if len(hit) else -1)
                                assert list(hit) == [first.value + k * S for k in range(len(hit))]  # consecutive members
                                n_hits[1 if want >= 0 else want] += 1
    assert min(n_hits.values()) > 50, n_hits  # none, one and several all occurred
    assert L.ccd_debug_lattice_stride(0, 8, 0, 0, 1, 1, 0, 0) == ERR_ARG and L.ccd_debug_lattice_stride(4, 8, 0, 0, 1, 0, 0, 0) == ERR_ARG
    assert L.ccd_debug_lattice_hit(4, 8, 0, 0, 1, 1, 0, 0, 0, 0, 1, None, None) == ERR_ARG
    assert L.ccd_latent_probe_stride_margin(C.byref(arches[0][1]), 0, 0, -1) == ERR_ARG


def _f32(v):
    return np.float32(v)


def _tap_interval(taps, f, i, n, g):
    """numpy restatement of the reference indices [a, b] the warp reads along one axis (n samples, global shift g) for sample
    i with the flow f: oracle/cc_oracle.c section 11, the sinc window and grid_sample's bilinear / bicubic."""
    f = _f32(f)

    def index(t):
        return int(np.clip(int(np.clip(t, 0, n - 1)) + g, 0, n - 1))

    if taps >= 6:
        first = i - taps // 2 + 1 + int(np.clip(np.floor(f), -(n + 16), n + 16))
    else:
        s = _f32((n - 1.0) / 2.0)
        if n == 1:
            lin = _f32(-1.0)
        else:
            step = _f32(2.0) / _f32(n - 1)
            lin = _f32(np.float64(step) * i - 1.0) if i < n // 2 else _f32(-np.float64(step) * (n - 1 - i) + 1.0)  # one rounding: an fma
        c = _f32(_f32(_f32(lin + _f32(f / s)) + _f32(1.0)) * s)
        if taps == 2:
            first = int(np.floor(np.clip(c, _f32(0.0), _f32(n - 1))))
        else:
            first = int(np.clip(np.floor(c), -4.0, n + 4.0)) - 1
    return index(first), index(first + taps - 1)


@pytest.mark.parametrize("frame_type", ["P", "B"])
@pytest.mark.parametrize("fdt", ["yuv444", "yuv420"])
@pytest.mark.parametrize("taps", [2, 4, 6, 8])
def test_reference_change_stays_inside_the_tap_windows(oracle, frame_type, fdt, taps):
    """The premise of section 4.16 against the oracle: changing ONE sample of a reference changes only samples of the dependent
    whose tap interval (both axes) holds it - for a 4:2:0 chroma sample, a window of one of the quad's four samples.  16 x 24,
    flows up to +-30 so that the clamps occur, a non-zero global flow."""
    h, w = 16, 24
    rng = np.random.default_rng([taps, int(frame_type == "B"), int(fdt == "yuv420"), 416])
    n_refs = 2 if frame_type == "B" else 1
    residue = rng.uniform(-0.2, 0.2, size=(3 + n_refs, h, w)).astype(np.float32)
    motion = rng.uniform(-3.0, 3.0, size=(2 * n_refs, h, w)).astype(np.float32)
    far = rng.random(size=motion.shape) < 0.15
    motion[far] = rng.uniform(-30.0, 30.0, size=int(far.sum())).astype(np.float32)
    half = fdt == "yuv420"
    cs = (h // 2, w // 2) if half else (h, w)
    refs = [[rng.integers(0, 256, size=s).astype(np.uint16) for s in ((h, w), cs, cs)] for _ in range(2)]
    gflow = [1, -1, -2, 3]

    def run(r):
        return oracle.inter_reconstruct(frame_type, residue, motion, r[0], r[1] if n_refs == 2 else None, gflow, taps, 8, fdt)

    base = run(refs)
    changed = 0
    for which in range(n_refs):
        win = np.zeros((h, w, 4), np.int64)  # ya, yb, xa, xb of every sample's window into reference `which`
        for y in range(h):
            for x in range(w):
                win[y, x, :2] = _tap_interval(taps, motion[2 * which + 1, y, x], y, h, gflow[2 * which + 1])
                win[y, x, 2:] = _tap_interval(taps, motion[2 * which, y, x], x, w, gflow[2 * which])
        for p, (y, x) in [(0, (7, 11)), (0, (0, 0)), (0, (h - 1, w - 1)), (1, (3, 5)), (2, (cs[0] - 1, 0)), (1, (0, cs[1] - 1)), (0, (9, 2)),
                            (0, (4, 17)), (0, (12, 6)), (2, (6, 9)), (0, (2, 20)), (1, (5, 2)), (0, (13, 13))]:
            r2 = [[a.copy() for a in r] for r in refs]
            r2[which][p][y, x] ^= 0x80
            # the changed samples of the 4:4:4 reference
            y0, y1, x0, x1 = (2 * y, 2 * y + 1, 2 * x, 2 * x + 1) if (p and half) else (y, y, x, x)
            reads = (win[..., 0] <= y1) & (win[..., 1] >= y0) & (win[..., 2] <= x1) & (win[..., 3] >= x0)
            quads = reads.reshape(h // 2, 2, w // 2, 2).any(axis=(1, 3))
            got = run(r2)
            for q in range(3):
                diff = got[q] != base[q]
                changed += int(diff.sum())
                allowed = quads if (q and half) else reads
                assert not (diff & ~allowed).any(), (frame_type, fdt, taps, which, p, y, x, q, np.argwhere(diff & ~allowed)[:4].tolist())
    assert changed >= 20  # the changes did move samples


# ---- GPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cool_chic_amd import DistortionDeltas, _lib

    _lib.lib()
    assert hasattr(DistortionDeltas, "add_dependent")
    return DistortionDeltas


def _entry(maps, mv):
    return int(maps[mv[0]][(mv[3] + 1) // 2, mv[1], mv[2]])


def _compare(name, maps, moves, want):
    bad = [(mv, _entry(maps, mv), w) for mv, w in zip(moves, want) if _entry(maps, mv) != w]
    assert not bad, (name, len(bad), len(moves), bad[:6])


def _sampled(ref, rng, n_random=24, grids=None):
    import inter_cases as ic

    return [(g, y, x, s) for g in (range(ref.n) if grids is None else grids) for y, x in ic.sample_positions(*ref.hw[g], rng, n_random)
            for s in (-1, 1)]


def _sentinels(ref, maps):
    for g in range(ref.n):
        assert np.array_equal(maps[g][0] == SENTINEL, ref.lat[g] == -64) and np.array_equal(maps[g][1] == SENTINEL, ref.lat[g] == 63), g


def _equal_maps(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def _shares(name, ref, moves, want, require=True):
    real = [w for mv, w in zip(moves, want) if w != SENTINEL and not ref.arch.is_hyperlatent[mv[0]]]
    nz = sum(1 for w in real if w != 0)
    print(f"{name}: {len(moves)} entries, {len(real)} legal on latent grids, {nz} non-zero ({nz / max(len(real), 1):.3f}), "
          f"{sum(1 for w in real if w < 0)} negative, {sum(1 for w in real if w > 0)} positive, dDdep in [{min(real)}, {max(real)}]")
    if require:
        assert 8 * nz >= len(real), (name, nz, len(real))
        assert min(real) < 0 < max(real)


@pytest.mark.gpu
def test_intra_frame_with_p_dependent(gpu):
    """vid3_ldp: the I frame with the P frame that predicts from it (sinc-8, yuv420 8-bit, the fixture's own outputs).  The in-quad
    tap offsets of the fixture's flows differ by at most 2, so no entry is a conflict; every entry of the three coarsest latent
    grids and sampled positions of the finer ones equal the brute force; sentinels, own maps, passes."""
    import dependent_cases as dc
    import inter_cases as ic

    ref = dc.intra("vid3_ldp")
    f = ic.case("vid3_ldp", 1)
    dep = dc.Dependent(f, 0)
    assert (f.taps, f.fdt, f.bd, f.gflow[:2]) == (8, 1, 8, [0, -2])
    spread = dc.quad_spread(dc.tap_offsets(dep.motion.cpu().numpy(), 0, f.H, f.W, f.taps))
    print("largest in-quad difference of the tap offsets:", spread)
    assert spread <= 2
    own, maps, conflicts, passes = dc.run_maps(gpu, ref, [dep])
    assert conflicts == [0] * ref.n
    latent = [g for g in range(ref.n) if not ref.arch.is_hyperlatent[g]]
    coarse = latent[-3:]
    rng = np.random.default_rng(21)
    moves = [(g, y, x, s) for g in coarse for y in range(ref.hw[g][0]) for x in range(ref.hw[g][1]) for s in (-1, 1)]
    moves += _sampled(ref, rng, grids=[g for g in range(ref.n) if g not in coarse])
    want = dc.brute(ref, [dep], moves)
    _shares(ref.name, ref, moves, want)
    _compare(ref.name, maps, moves, want)
    _sentinels(ref, maps)
    for g in range(ref.n):
        assert maps[g].shape == (2,) + ref.hw[g] and maps[g].dtype == np.int64
        if ref.arch.is_hyperlatent[g]:
            assert not maps[g][maps[g] != SENTINEL].any()
    alone, none, _, passes_alone = dc.run_maps(gpu, ref, [])
    assert none is None and _equal_maps(own, alone)
    m = dc.margin(ref.fdt, [f.taps])
    assert m == 10 and passes == dc.expected_passes(ref, m) and passes_alone == dc.expected_passes(ref, 0) and passes > passes_alone


@pytest.mark.gpu
@pytest.mark.parametrize("role", ["residue", "motion"])
def test_inter_reference(gpu, role):
    """vid3_ldp frame 1 (P) is the reference of frame 2: each of its cool-chics as the candidate, sampled entries."""
    import dependent_cases as dc
    import inter_cases as ic

    assert ic.parse_video("vid3_ldp")[2][3] == [1]
    ref = dc.InterRef(ic.case("vid3_ldp", 1), role)
    dep = dc.Dependent(ic.case("vid3_ldp", 2), 0)
    own, maps, conflicts, _ = dc.run_maps(gpu, ref, [dep])
    assert conflicts == [0] * ref.n
    moves = _sampled(ref, np.random.default_rng(22), n_random=8)
    want = dc.brute(ref, [dep], moves)
    _shares(ref.name, ref, moves, want)
    _compare(ref.name, maps, moves, want)
    assert _equal_maps(own, ref.case.maps(role))


@pytest.mark.gpu
def test_b_dependents(gpu):
    """vid5: the I frame is reference 0 of two B frames (coding indices 2 and 3) - each alone, and both on one slot, whose map is
    the sum of the two; the B frame of coding index 2 is reference 1 of coding index 3."""
    import dependent_cases as dc
    import inter_cases as ic

    video = ic.parse_video("vid5")
    assert video[2][3][0] == video[0][2] and video[3][3] == [video[0][2], video[2][2]]
    ref = dc.intra("vid5")
    deps = [dc.Dependent(ic.case("vid5", 2), 0), dc.Dependent(ic.case("vid5", 3), 0)]
    moves = _sampled(ref, np.random.default_rng(23), n_random=8)
    single = []
    for dep in deps:
        _, maps, conflicts, _ = dc.run_maps(gpu, ref, [dep])
        assert conflicts == [0] * ref.n
        want = dc.brute(ref, [dep], moves)
        _shares(ref.name + " <- " + dep.case.name, ref, moves, want)
        _compare(dep.case.name, maps, moves, want)
        single.append(maps)
    _, both, conflicts, _ = dc.run_maps(gpu, ref, deps)
    assert conflicts == [0] * ref.n
    for g in range(ref.n):
        legal = single[0][g] != SENTINEL
        assert np.array_equal(both[g] != SENTINEL, legal)
        assert np.array_equal(both[g][legal], single[0][g][legal] + single[1][g][legal]), g
    # reference 1: the residue cool-chic of the B frame at coding index 2, read by coding index 3
    ref1 = dc.InterRef(ic.case("vid5", 2), "residue")
    dep1 = dc.Dependent(ic.case("vid5", 3), 1)
    _, maps, conflicts, _ = dc.run_maps(gpu, ref1, [dep1])
    assert conflicts == [0] * ref1.n
    moves = _sampled(ref1, np.random.default_rng(24), n_random=8)
    want = dc.brute(ref1, [dep1], moves)
    _shares(ref1.name + " <- which 1", ref1, moves, want)
    _compare(ref1.name, maps, moves, want)


def _random_flows(case, rng, amplitude, per_quad):
    import torch

    H, W = case.H, case.W
    if per_quad:
        m = rng.uniform(-amplitude, amplitude, size=(2, H // 2, W // 2)).astype(np.float32).repeat(2, axis=1).repeat(2, axis=2)
    else:
        m = rng.uniform(-amplitude, amplitude, size=(2, H, W)).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(m)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("fdt,bitdepth,per_quad", [(0, 8, False), (2, 10, False), (1, 8, True)])
@pytest.mark.parametrize("taps", [2, 4, 6, 8])
def test_long_range_scatter_without_conflicts(gpu, fdt, bitdepth, per_quad, taps):
    """Flows uniform in +-20 and a global flow: the change of one latent lands far from its box.  rgb 8-bit and yuv444 10-bit with a
    flow per sample, yuv420 with a flow per 2 x 2 quad: by the margin's rule no entry is a conflict, and sampled entries equal the
    brute force."""
    import dependent_cases as dc
    import inter_cases as ic

    ref = dc.intra("vid3_ldp", formats=(fdt, bitdepth))
    f = ic.case("vid3_ldp", 1, formats=(fdt, bitdepth), warp_filter_size=taps)
    rng = np.random.default_rng([25, fdt, taps])
    dep = dc.Dependent(f, 0, motion=_random_flows(f, rng, 20.0, per_quad), gflow=[3, -5, 0, 0])
    _, maps, conflicts, passes = dc.run_maps(gpu, ref, [dep])
    assert conflicts == [0] * ref.n
    assert passes == dc.expected_passes(ref, dc.margin(fdt, [taps]))
    moves = _sampled(ref, rng, n_random=4)
    want = dc.brute(ref, [dep], moves)
    _shares(f"{ref.name} fdt {fdt} taps {taps}", ref, moves, want)
    _compare((fdt, taps), maps, moves, want)
    assert all(m != SENTINEL for m, w in zip([_entry(maps, mv) for mv in moves], want) if w != SENTINEL)


@pytest.mark.gpu
def test_conflicts_are_flagged(gpu):
    """yuv420 with a random flow per SAMPLE (+-3: tap offsets inside a quad differ by up to 6): quads read the regions of two
    latents, those entries are flagged and counted; every sampled entry that is not flagged equals the brute force, and at least a
    quarter of the sampled legal entries are not flagged."""
    import dependent_cases as dc
    import inter_cases as ic

    ref = dc.intra("vid3_ldp")
    f = ic.case("vid3_ldp", 1)
    rng = np.random.default_rng(26)
    dep = dc.Dependent(f, 0, motion=_random_flows(f, rng, 3.0, False), gflow=[1, -2, 0, 0])
    _, maps, conflicts, _ = dc.run_maps(gpu, ref, [dep])
    print("conflicts per grid:", conflicts)
    assert sum(conflicts) > 0
    for g in range(ref.n):
        legal = np.stack([ref.lat[g] != -64, ref.lat[g] != 63])
        assert int(((maps[g] == SENTINEL) & legal).sum()) == conflicts[g], g
    moves = _sampled(ref, rng, n_random=8)
    want = dc.brute(ref, [dep], moves)
    legal = [(mv, w) for mv, w in zip(moves, want) if w != SENTINEL]
    free = [(mv, w) for mv, w in legal if _entry(maps, mv) != SENTINEL]
    print(f"{len(free)} of {len(legal)} sampled legal entries are not flagged ({len(free) / len(legal):.3f})")
    assert 4 * len(free) >= len(legal)
    bad = [(mv, _entry(maps, mv), w) for mv, w in free if _entry(maps, mv) != w]
    assert not bad, (len(bad), bad[:6])
    assert all(_entry(maps, mv) == SENTINEL for mv, w in zip(moves, want) if w == SENTINEL)


@pytest.mark.gpu
def test_invariances(gpu):
    """The maps are the same for 3 and 16 probe slots and with an unrelated slot in the handle; after latents are changed in place
    and the dependent's motion buffer is rewritten, a second run follows both and equals a fresh handle."""
    import torch

    import dependent_cases as dc
    import inter_cases as ic

    ref = dc.intra("vid3_ldp")
    f, other = ic.case("vid3_ldp", 1), ic.case("vid3_ldp", 2)
    dep = dc.Dependent(f, 0)
    own16, maps16, conf16, passes16 = dc.run_maps(gpu, ref, [dep], n_probe_slots=16)
    own3, maps3, conf3, passes3 = dc.run_maps(gpu, ref, [dep], n_probe_slots=3)
    assert _equal_maps(maps3, maps16) and _equal_maps(own3, own16) and conf3 == conf16 and passes3 == passes16
    own_x, maps_x, conf_x, _ = dc.run_maps(gpu, ref, [dep], extra=lambda d: other.add_to(d, "motion"))
    assert _equal_maps(maps_x, maps16) and _equal_maps(own_x, own16) and conf_x == conf16
    # in place: new latents in the candidate's device buffer, new flows in the dependent's motion buffer
    lat_dev = ref.cc.lat_dev.clone()
    motion = dep.motion.clone()
    d = gpu(0, 16)
    slot = ref.add_to(d, lat_dev=lat_dev)
    dep.add_to(d, slot, motion=motion)
    d.run(); d.wait()
    first = [torch.as_tensor(d.dep_delta_map(slot, g), device="cuda").cpu().numpy() for g in range(ref.n)]
    assert _equal_maps(first, maps16)
    lat_dev.copy_(torch.from_numpy(ref.cc.flat(ref.cc.lat2)).cuda())
    motion.add_(0.75)
    torch.cuda.synchronize()
    d.run(); d.wait()
    second = [torch.as_tensor(d.dep_delta_map(slot, g), device="cuda").cpu().numpy() for g in range(ref.n)]
    d.close()
    fresh = gpu(0, 16)
    slot = ref.add_to(fresh, lat_dev=lat_dev)
    dep.add_to(fresh, slot, motion=motion)
    fresh.run(); fresh.wait()
    want = [torch.as_tensor(fresh.dep_delta_map(slot, g), device="cuda").cpu().numpy() for g in range(ref.n)]
    fresh.close()
    assert _equal_maps(second, want) and not _equal_maps(second, first)
    moves = _sampled(ref, np.random.default_rng(27), n_random=2, grids=[0, 3])
    _compare("followed", second, moves, dc.brute(ref, [dep], moves, lat=ref.cc.lat2, motions=[motion]))


@pytest.mark.gpu
def test_one_move_end_to_end(gpu):
    """RdEvaluator: the argmin of cost_delta_map(dependents=True) on grid 0, applied as ONE move to the device latents, changes
    SSE_R + SSE_F by exactly own + dep of that entry."""
    import torch

    import dependent_cases as dc
    import inter_cases as ic
    from cool_chic_amd.io import FrameData
    from cool_chic_amd.quality import QualityMeter
    from cool_chic_amd.rd import RdEvaluator

    ref = dc.intra("vid3_ldp")
    dep = dc.Dependent(ic.case("vid3_ldp", 1), 0)
    lat_dev = ref.cc.lat_dev.clone()
    src = [p.cpu().numpy() for p in ref.src]
    source = FrameData(8, "yuv420", {"y": torch.from_numpy(src[0].astype(np.float32) / 255.0)[None, None],
                                     "u": torch.from_numpy(src[1].astype(np.float32) / 255.0)[None, None],
                                     "v": torch.from_numpy(src[2].astype(np.float32) / 255.0)[None, None]})

    def sse_f(planes):
        with QualityMeter(0) as meter:
            r, = meter.score_planes([dep.reconstruct(planes)], [dep.src], [8], ["yuv420"], ms_ssim=False)
        return sum(int(v) for v in r.sse)

    with RdEvaluator(0) as ev:
        slot = ev.add(ref.arch, ref.nn, ref.cc.ptrs(lat_dev), source, owner=lat_dev)
        ev.add_dependent(slot, dep.case.frame_type, 0, dep.residue.data_ptr(), dep.motion.data_ptr(), [t.data_ptr() for t in dep.src],
                         None, dep.gflow, dep.case.taps, owner=dep)
        lmbda = 1e-3
        before = ev.evaluate(lmbda, rate_deltas=True, distortion_deltas=True)[0]
        planes0 = [torch.as_tensor(ev._dec.plane_device(slot, p), device="cuda").clone() for p in range(3)]
        f_before = sse_f(planes0)
        cost = ev.cost_delta_map(slot, 0, lmbda, dependents=True)
        plain = ev.cost_delta_map(slot, 0, lmbda)
        own = torch.as_tensor(ev.distortion_delta_map(slot, 0), device="cuda").cpu().numpy()
        depm = torch.as_tensor(ev.dependent_delta_map(slot, 0), device="cuda").cpu().numpy()
        assert torch.equal(torch.isinf(cost).cpu(), torch.from_numpy((own == SENTINEL) | (depm == SENTINEL)))
        assert not torch.equal(cost, plain)
        k = int(torch.argmin(cost))
        h, w = ref.hw[0]
        s, y, x = k // (h * w), (k % (h * w)) // w, k % w
        assert own[s, y, x] != SENTINEL and depm[s, y, x] != SENTINEL
        lat_dev[int(ref.cc.off[0]) + y * w + x] += 2 * s - 1
        torch.cuda.synchronize()
        after = ev.evaluate(lmbda)[0]
        planes1 = [torch.as_tensor(ev._dec.plane_device(slot, p), device="cuda").clone() for p in range(3)]
        f_after = sse_f(planes1)
    d_r = sum(int(v) for v in after.quality.sse) - sum(int(v) for v in before.quality.sse)
    print("move", (s, y, x), "own", int(own[s, y, x]), "dep", int(depm[s, y, x]), "dSSE_R", d_r, "dSSE_F", f_after - f_before)
    assert d_r == int(own[s, y, x]) and f_after - f_before == int(depm[s, y, x])
    assert d_r + f_after - f_before == int(own[s, y, x]) + int(depm[s, y, x])
