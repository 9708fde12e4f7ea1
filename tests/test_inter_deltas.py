"""Distortion deltas of P / B frames (ccd_dsens_add_inter, DistortionDeltas.add_inter): for every latent
of one of the frame's two cool-chics the exact change of the FRAME's squared error if that latent were v - 1 or v + 1, the other
cool-chic's output and the references held fixed.

The reference is brute force from calls other test files pin (tests/inter_cases.py): one latent moved on the host,
DecodeBatch.add_latents* with the float output kept, ccd_inter_reconstruct with the partner's base output, QualityMeter.score_planes,
minus the base SSE.  Everything is compared as integers; the distortion side has no tolerance."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

ERR_VALUE, ERR_ARG = -2, -7
SENTINEL = -2 ** 63


# ---- CPU -------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound():
    from cool_chic_amd import _lib

    with open(os.path.join(ROOT, "include", "ccd.h")) as f:
        header = f.read()
    assert "ccd_dsens_add_inter(" in header and "} ccd_dsens_inter;" in header
    assert "ccd_dsens_add_inter" in _lib.SIGNATURES
    assert getattr(_lib.lib(), "ccd_dsens_add_inter") is not None
    import cool_chic_amd

    assert hasattr(cool_chic_amd.DistortionDeltas, "add_inter")


def _inter(frame_type=1, role=0, partner=1, ref0=(1, 1, 1), ref1=(0, 0, 0), taps=8):
    from cool_chic_amd._lib import DsensInter

    return DsensInter(frame_type=frame_type, role=role, partner=partner or None, ref0=(C.c_void_p * 3)(*[p or None for p in ref0]),
                      ref1=(C.c_void_p * 3)(*[p or None for p in ref1]), global_flow=(C.c_int32 * 4)(0, 0, 0, 0), warp_filter_size=taps)


def test_argument_errors_without_a_device():
    """Every refusal comes before the handle's batch or the device is looked at: the handle is 1 KiB of zeros, the buffers are
    host arrays whose addresses only stand for device pointers."""
    import inter_cases as ic
    from cool_chic_amd._lib import CCHeader, lib

    L = lib()
    _, ccs, _, _ = ic.parse_video("vid3_ldp")[1]
    (res, _, res_nn, _), (mot, _, mot_nn, _) = ccs
    assert (res.out_channels, mot.out_channels) == (4, 2)
    handle = C.create_string_buffer(1024)
    d = C.cast(handle, C.c_void_p)
    grid = np.zeros(128 * 224, np.int8)
    a = grid.ctypes.data
    lat = (C.c_void_p * 40)(*[a] * 40)
    src = (C.c_void_p * 3)(a, a, a)

    def add(arch=res, nn=res_nn, handle=d, latents=lat, source=src, bitdepth=8, fdt=1, inter="default", **kw):
        it = _inter(**{"partner": a, "ref0": (a, a, a), **kw}) if inter == "default" else inter
        return L.ccd_dsens_add_inter(handle, C.byref(arch) if arch is not None else None, nn, len(nn) if nn else 0, latents, source,
                                     bitdepth, fdt, C.byref(it) if it is not None else None)

    # CCD_ERR_ARG
    assert add(handle=None) == ERR_ARG and add(arch=None) == ERR_ARG and add(nn=None) == ERR_ARG
    assert add(latents=None) == ERR_ARG and add(source=None) == ERR_ARG
    assert add(source=(C.c_void_p * 3)(a, None, a)) == ERR_ARG
    assert add(inter=None) == ERR_ARG
    assert add(partner=0) == ERR_ARG
    for p in range(3):
        ref = [a, a, a]
        ref[p] = 0
        assert add(ref0=tuple(ref)) == ERR_ARG
        assert add(frame_type=2, ref1=tuple(ref)) == ERR_ARG      # a B frame needs its second reference
    for frame_type in (0, 3, -1):
        assert add(frame_type=frame_type) == ERR_ARG
    for role in (-1, 2):
        assert add(role=role) == ERR_ARG
    for bitdepth in (0, 7, 17):
        assert add(bitdepth=bitdepth) == ERR_ARG
    assert add(fdt=3) == ERR_ARG and add(fdt=-1) == ERR_ARG
    pending = C.create_string_buffer(1024)  # a run in flight: whatever the handle holds says so
    pending.raw = b"\x01" * 1024
    assert add(handle=C.cast(pending, C.c_void_p)) == ERR_ARG
    # CCD_ERR_VALUE
    for taps in (0, 1, 3, 7, 18, -2):
        assert add(taps=taps) == ERR_VALUE, taps
    odd = CCHeader.from_buffer_copy(bytes(res))
    odd.img_size[0] = 127
    assert add(arch=odd) == ERR_VALUE                             # yuv420 with an odd side
    assert add(arch=mot, nn=mot_nn, role=0) == ERR_VALUE          # 2 channels are no residue
    assert add(role=1) == ERR_VALUE                               # 4 channels are no P frame's motion
    assert add(frame_type=2, ref1=(a, a, a)) == ERR_VALUE         # a B frame's residue has 5 channels
    assert add(arch=mot, nn=mot_nn, role=1, frame_type=2, ref1=(a, a, a)) == ERR_VALUE  # and its motion 4
    assert bytes(handle) == bytes(1024)


@pytest.mark.parametrize("frame_type", ["P", "B"])
@pytest.mark.parametrize("fdt", ["yuv444", "yuv420"])
@pytest.mark.parametrize("taps", [2, 4, 6, 8])
def test_reconstruction_is_pointwise(oracle, frame_type, fdt, taps):
    """The premise of section 4.15 against the oracle: changing the residue, alpha (beta) or the flow at ONE pixel changes at most
    that luma sample and the chroma sample that holds it.  16 x 24, an interior pixel, a corner and an edge."""
    h, w = 16, 24
    rng = np.random.default_rng([taps, int(frame_type == "B"), int(fdt == "yuv420")])
    n_refs = 2 if frame_type == "B" else 1
    residue = rng.uniform(-0.2, 0.2, size=(3 + n_refs, h, w)).astype(np.float32)
    motion = rng.uniform(-3.0, 3.0, size=(2 * n_refs, h, w)).astype(np.float32)
    cs = (h // 2, w // 2) if fdt == "yuv420" else (h, w)
    refs = [[rng.integers(0, 256, size=s).astype(np.uint16) for s in ((h, w), cs, cs)] for _ in range(2)]
    gflow = [1, -1, -2, 0]

    def run(res, mot):
        return oracle.inter_reconstruct(frame_type, res, mot, refs[0], refs[1] if n_refs == 2 else None, gflow, taps, 8, fdt)

    base = run(residue, motion)
    changed = 0
    for y, x in [(7, 11), (0, 0), (h - 1, w - 1), (0, 13), (9, w - 1)]:
        variants = []
        for c in range(3 + n_refs):           # residue channels, alpha, beta
            r2 = residue.copy()
            r2[c, y, x] += 0.3
            variants.append((r2, motion))
        for c in range(2 * n_refs):           # flows
            m2 = motion.copy()
            m2[c, y, x] += 1.37
            variants.append((residue, m2))
        r2, m2 = residue.copy(), motion.copy()  # everything at once
        r2[:, y, x] -= 0.25
        m2[:, y, x] -= 2.6
        variants.append((r2, m2))
        for res, mot in variants:
            got = run(res, mot)
            for p in range(3):
                diff = got[p] != base[p]
                changed += int(diff.sum())
                if p and fdt == "yuv420":
                    diff[y // 2, x // 2] = False
                else:
                    diff[y, x] = False
                assert not diff.any(), (frame_type, fdt, taps, y, x, p, np.argwhere(diff)[:4].tolist())
    assert changed > 20  # the changes did move samples


# ---- GPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cool_chic_amd import DistortionDeltas, _lib

    _lib.lib()
    assert hasattr(DistortionDeltas, "add_inter")
    return DistortionDeltas


def _entry(maps, mv):
    return int(maps[mv[0]][(mv[3] + 1) // 2, mv[1], mv[2]])


def _compare(case, role, maps, moves, want):
    bad = [(mv, _entry(maps, mv), w) for mv, w in zip(moves, want) if _entry(maps, mv) != w]
    assert not bad, (case.name, role, len(bad), len(moves), bad[:6])


def _shares(case, role, moves, want, require=True):
    """The condition on the REFERENCE values alone: of the legal brute-force entries of the non-hyperlatent grids at least a
    quarter are non-zero, and both signs occur."""
    arch = case.cc[role].arch
    real = [w for mv, w in zip(moves, want) if w != SENTINEL and not arch.is_hyperlatent[mv[0]]]
    nz = sum(1 for w in real if w != 0)
    print(f"{case.name} {role}: {len(moves)} entries, {len(real)} legal on latent grids, {nz} non-zero ({nz / max(len(real), 1):.3f}), "
          f"{sum(1 for w in real if w < 0)} negative, {sum(1 for w in real if w > 0)} positive, dD in [{min(real)}, {max(real)}]")
    if require:
        assert 4 * nz >= len(real), (case.name, role, nz, len(real))
        assert min(real) < 0 < max(real)


def _sentinels(case, role, maps):
    cc = case.cc[role]
    for g in range(cc.n):
        assert np.array_equal(maps[g][0] == SENTINEL, cc.lat[g] == -64) and np.array_equal(maps[g][1] == SENTINEL, cc.lat[g] == 63), (role, g)


def _sampled_moves(case, role, rng, n_random=24, grids=None):
    import inter_cases as ic

    cc = case.cc[role]
    return [(g, y, x, s) for g in (range(cc.n) if grids is None else grids) for y, x in ic.sample_positions(*cc.hw[g], rng, n_random)
            for s in (-1, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("role", ["residue", "motion"])
def test_p_frame_every_coarse_latent(gpu, role):
    """vid3_ldp frame 1 (P, yuv420 8-bit, sinc-8): EVERY latent and both signs of the three coarsest latent grids (8 x 14, 4 x 7,
    2 x 4: smaller than their stride, boxes clipped on every side, boxes that are the whole picture), sampled positions on the finer
    ones, the hyperlatent grids of the residue cool-chic, the sentinels of every map."""
    import inter_cases as ic

    case = ic.case("vid3_ldp", 1)
    cc = case.cc[role]
    maps = case.maps(role)
    latent = [g for g in range(cc.n) if not cc.arch.is_hyperlatent[g]]
    coarse = latent[-3:]
    assert [cc.hw[g] for g in coarse] == [(8, 14), (4, 7), (2, 4)] and (role == "residue" or coarse == [2, 3, 4])
    rng = np.random.default_rng(7)
    moves = [(g, y, x, s) for g in coarse for y in range(cc.hw[g][0]) for x in range(cc.hw[g][1]) for s in (-1, 1)]
    moves += _sampled_moves(case, role, rng, grids=[g for g in range(cc.n) if g not in coarse])
    want = case.brute(role, moves)
    _shares(case, role, moves, want)
    _compare(case, role, maps, moves, want)
    _sentinels(case, role, maps)
    n_hyper = 0
    for g in range(cc.n):
        if cc.arch.is_hyperlatent[g]:  # does not feed the synthesis: zeros, and the sentinel at the alphabet's ends
            n_hyper += 1
            assert not maps[g][maps[g] != SENTINEL].any()
    assert n_hyper == (3 if role == "residue" else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("role", ["residue", "motion"])
def test_b_frame_sampled(gpu, role):
    """vid5, coding index 2 (B): the second reference, beta, a 4-channel motion output."""
    import inter_cases as ic

    case = ic.case("vid5", 2)
    assert case.frame_type == 2 and case.cc["residue"].arch.out_channels == 5 and case.cc["motion"].arch.out_channels == 4
    maps = case.maps(role)
    moves = _sampled_moves(case, role, np.random.default_rng(8))
    want = case.brute(role, moves)
    _shares(case, role, moves, want)
    _compare(case, role, maps, moves, want)
    _sentinels(case, role, maps)


@pytest.mark.gpu
@pytest.mark.parametrize("name,index,taps", [("vid5_w2", 3, None), ("vid5_w4", 4, None), ("vid3_ldp", 1, 6)])
def test_other_warp_filters(gpu, name, index, taps):
    """The native 2- and 4-tap paths (two B frames; the streams' one P frame has a global flow of (256, 256), reads the border
    everywhere and has no motion deltas but 0) and a run-time sinc size, 6, obtained by changing only warp_filter_size in the call;
    the motion role, whose probes warp."""
    import inter_cases as ic

    case = ic.case(name, index) if taps is None else ic.case(name, index, warp_filter_size=taps)
    assert case.taps == (taps or int(name[-1]))
    maps = case.maps("motion")
    moves = _sampled_moves(case, "motion", np.random.default_rng(9))
    want = case.brute("motion", moves)
    _shares(case, "motion", moves, want)
    _compare(case, "motion", maps, moves, want)
    _sentinels(case, "motion", maps)


@pytest.mark.gpu
@pytest.mark.parametrize("fdt,bitdepth", [(0, 8), (2, 10)])
@pytest.mark.parametrize("role", ["residue", "motion"])
def test_formats(gpu, role, fdt, bitdepth):
    """The P cool-chics of vid3_ldp as an rgb 8-bit and a yuv444 10-bit frame over seeded random reference planes: u16 planes,
    no chroma halving.  16 positions per grid."""
    import inter_cases as ic

    case = ic.case("vid3_ldp", 1, formats=(fdt, bitdepth))
    maps = case.maps(role)
    moves = _sampled_moves(case, role, np.random.default_rng(10), n_random=8)
    want = case.brute(role, moves)
    _shares(case, role, moves, want)
    _compare(case, role, maps, moves, want)
    _sentinels(case, role, maps)


def _equal_maps(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
def test_independence(gpu):
    """The motion maps of vid3_ldp frame 1 do not depend on the number of probe slots, nor on what else the handle holds: an
    intra candidate (odd18x65 through ccd_dsens_add), the frame's residue candidate and both candidates of frame 2.  The intra
    candidate's maps are those of a handle that holds it alone."""
    import inter_cases as ic
    from test_distortion_deltas import _case as intra_case

    case, other = ic.case("vid3_ldp", 1), ic.case("vid3_ldp", 2)
    want = case.maps("motion")
    d = gpu(0, 3)
    case.add_to(d, "motion")
    d.run(); d.wait()
    assert _equal_maps(case.read_maps(d, 0, "motion"), want)
    n_passes = d.passes(0)
    d.close()
    intra = intra_case("odd18x65")
    intra_want = intra.maps(gpu)
    d = gpu(0, 16)
    slots = {"intra": d.add(intra.arch, intra.nn, intra.ptrs(intra.lat_dev), [t.data_ptr() for t in intra.src], intra.bd, intra.fdt,
                            owner=(intra.lat_dev, intra.src))}
    slots["residue"] = case.add_to(d, "residue")
    slots["motion"] = case.add_to(d, "motion")
    slots["other residue"] = other.add_to(d, "residue")
    slots["other motion"] = other.add_to(d, "motion")
    assert d.passes(slots["motion"]) == n_passes  # counted as before: 2 * sum of min(S, h) * min(S, w)
    for run in range(2):
        d.run(); d.wait()
        assert _equal_maps(case.read_maps(d, slots["motion"], "motion"), want), run
        assert _equal_maps(intra.run_maps(d, slots["intra"]), intra_want), run
        assert _equal_maps(case.read_maps(d, slots["residue"], "residue"), case.maps("residue")), run
    d.close()


@pytest.mark.gpu
def test_two_filter_sizes_in_one_handle(gpu):
    """A handle whose candidates use the sinc-8 warp AND another filter size reconstructs each round with two launches, one per
    kernel instantiation: the maps of both are those of handles that hold them alone."""
    import inter_cases as ic

    eight, six, two = ic.case("vid3_ldp", 1), ic.case("vid3_ldp", 1, warp_filter_size=6), ic.case("vid5_w2", 3)
    d = gpu(0, 16)
    held = [(six, "motion"), (eight, "motion"), (two, "residue"), (eight, "residue"), (six, "residue")]
    slots = [c.add_to(d, role) for c, role in held]
    d.run(); d.wait()
    for s, (c, role) in zip(slots, held):
        assert _equal_maps(c.read_maps(d, s, role), c.maps(role)), (c.name, c.taps, role)
    assert not _equal_maps(eight.maps("motion"), six.maps("motion"))
    d.close()


@pytest.mark.gpu
def test_followed_in_place(gpu):
    """Base latents changed on the device, and the partner's buffer overwritten, are followed by the next run; a base latent of
    100 is that slot's CCD_ERR_VALUE and leaves the other slot's maps intact."""
    import torch

    import inter_cases as ic
    from cool_chic_amd._lib import CcdError

    case = ic.case("vid3_ldp", 1)
    res, mot = case.cc["residue"], case.cc["motion"]
    lat_dev = res.lat_dev.clone()
    partner = case.out["residue"].clone()  # what the motion slot reads as the residue cool-chic's output
    d = gpu(0, 16)
    flows = case.out["motion"].clone()     # what the residue slot reads as the motion cool-chic's output
    s_res = case.add_to(d, "residue", lat_dev=lat_dev, partner=flows)
    s_mot = case.add_to(d, "motion", partner=partner)
    d.run(); d.wait()
    assert _equal_maps(case.read_maps(d, s_res, "residue"), case.maps("residue"))
    assert _equal_maps(case.read_maps(d, s_mot, "motion"), case.maps("motion"))
    # three base latents of the residue cool-chic
    lat_b = [a.copy() for a in res.lat]
    for g, y, x, v in [(0, 60, 100, 5), (2, 10, 20, -3), (4, 3, 7, 2)]:
        lat_b[g][y, x] = v
    lat_dev.copy_(torch.from_numpy(res.flat(lat_b)))
    torch.cuda.synchronize()
    d.run(); d.wait()
    maps_b = case.read_maps(d, s_res, "residue")
    assert not _equal_maps(maps_b, case.maps("residue"))
    rng = np.random.default_rng(11)
    moves = [mv for mv in _sampled_moves(case, "residue", rng, n_random=0) if mv[1:3] != (0, 0)][::3]
    moves += [(0, 60, 100, 1), (2, 10, 20, -1), (4, 3, 7, 1)]
    _compare(case, "residue", maps_b, moves, case.brute("residue", moves, lat=lat_b))
    assert _equal_maps(case.read_maps(d, s_mot, "motion"), case.maps("motion"))  # (its partner is a buffer of its own)
    # the partner's buffer: the residue output of the second latent set
    partner.copy_(case.out2["residue"])
    torch.cuda.synchronize()
    d.run(); d.wait()
    maps_m = case.read_maps(d, s_mot, "motion")
    assert not _equal_maps(maps_m, case.maps("motion"))
    moves = _sampled_moves(case, "motion", rng, n_random=0)[::2]
    _compare(case, "motion", maps_m, moves, case.brute("motion", moves, partner=case.out2["residue"]))
    # the residue slot's partner, the flows: the warped references it keeps are those of THIS run's base job
    flows.copy_(case.out2["motion"])
    torch.cuda.synchronize()
    d.run(); d.wait()
    maps_f = case.read_maps(d, s_res, "residue")
    assert not _equal_maps(maps_f, maps_b)
    moves = _sampled_moves(case, "residue", rng, n_random=0)[::3]
    _compare(case, "residue", maps_f, moves, case.brute("residue", moves, lat=lat_b, partner=case.out2["motion"]))
    flows.copy_(case.out["motion"])
    torch.cuda.synchronize()
    d.run(); d.wait()
    assert _equal_maps(case.read_maps(d, s_res, "residue"), maps_b)
    # outside the alphabet
    bad = res.flat(lat_b)
    bad[int(res.off[1]) + 5] = 100
    lat_dev.copy_(torch.from_numpy(bad))
    torch.cuda.synchronize()
    d.run()
    with pytest.raises(CcdError) as e:
        d.wait()
    assert e.value.code == ERR_VALUE
    with pytest.raises(CcdError) as e:
        d.delta_map(s_res, 0)
    assert e.value.code == ERR_VALUE
    assert _equal_maps(case.read_maps(d, s_mot, "motion"), maps_m)
    lat_dev.copy_(torch.from_numpy(res.flat(lat_b)))  # repaired: fine again
    torch.cuda.synchronize()
    d.run(); d.wait()
    assert _equal_maps(case.read_maps(d, s_res, "residue"), maps_b) and _equal_maps(case.read_maps(d, s_mot, "motion"), maps_m)
    d.close()


# ---- InterRdEvaluator and the tool ---------------------------------------------------------------------------------------
TERM_TOL = 24.0 * 2.0 ** -48  # the project's bound per log2 term of the rate meter (tests/test_device_rate.py)
# arm.py:501-509: priority of each of the 40 causal positions of the 9 x 9 mask, row-major; the k-th context is the position of rank k
PRIORITY = [38, 35, 30, 25, 23, 31, 36, 37, 39, 33, 28, 21, 20, 6, 15, 22, 29, 34, 32, 18,
            12, 10, 5, 9, 14, 19, 27, 24, 13, 8, 2, 1, 3, 11, 17, 26, 16, 7, 4, 0]


def _n_dep(arch, m, y, x):
    """How many symbols besides its own read the latent (m, y, x): its spatial dependents and the IFCE blocks of the finer grids
    (tests/test_rdoq.py::_Geo, restated from the architecture)."""
    n = int(arch.n_grids)
    hw = [(int(arch.grid_h[g]), int(arch.grid_w[g])) for g in range(n)]
    level = [0] * n
    for g in range(1, n):
        level[g] = level[g - 1] + (hw[g] != hw[g - 1])
    taps = [(4 - pos // 9, pos % 9 - 4) for pos, rank in enumerate(PRIORITY) if rank < int(arch.spatial_context_arm)]
    h, w = hw[m]
    dep = sum(1 for dy, dx in taps if 0 <= y + dy < h and 0 <= x - dx < w)
    for g in range(m):
        n_in = int(arch.input_features_ifce[g])
        if n_in > 0 and g != n - 1 and m - g - 1 < n_in:
            side = 2 << (level[m] - level[g + 1])
            gh, gw = hw[g]
            r1, c1 = min((y + 1) * side, gh) - 1, min((x + 1) * side, gw) - 1
            if y * side <= r1 and x * side <= c1:
                dep += (r1 - y * side + 1) * (c1 - x * side + 1)
    return dep


def _step_bound(ev, frame, role, arch, n_symbols):
    """tests/test_rdoq.py::_step_bound restated: the bound on |new total_bits - old - d_bits| of the step that just ran, from its
    move maps and the rate maps it read: sum over the moves of 2 (1 + |dep(p)|) TERM_TOL + |dBits(p)| 2^-23, plus 2 n_symbols
    TERM_TOL."""
    import torch

    bound, n = 2.0 * n_symbols * TERM_TOL, 0
    for g in range(int(arch.n_grids)):
        mv = torch.as_tensor(ev.step_moves(frame, role, g), device="cuda").cpu().numpy()
        db = torch.as_tensor(ev.rate_delta_map(frame, role, g), device="cuda").cpu().numpy()
        for y, x in zip(*np.nonzero(mv)):
            bound += 2.0 * (1 + _n_dep(arch, g, int(y), int(x))) * TERM_TOL + abs(float(db[(int(mv[y, x]) + 1) // 2, y, x])) * 2.0 ** -23
            n += 1
    return bound, n


def _frame_data(planes, bitdepth, fdt):
    from cool_chic_amd.quality import _planes_to_frame_data

    return _planes_to_frame_data([p.cpu().numpy() for p in planes], bitdepth, ic_fdt(fdt))


def ic_fdt(fdt):
    import inter_cases as ic

    return ic.FDT_NAMES[fdt]


@pytest.mark.gpu
def test_evaluator_on_the_fixture_latents(gpu):
    """evaluate() of vid3_ldp frames 1 and 2 (frame 2 predicts from frame 1) with the fixture's own latents: the planes are
    decode_video's, the bits the sum of EncodeBatch.measure of the two cool-chics, cost_delta_map the formula over the two maps."""
    import torch

    import inter_cases as ic
    from cool_chic_amd import DecodeBatch, EncodeBatch, InterRdEvaluator

    parsed = ic.parse_video("vid3_ldp")
    decoded = ic.decoded_planes("vid3_ldp")
    lmbda = 1e-3
    ev, enc, dec = InterRdEvaluator(0), EncodeBatch(0), DecodeBatch(0)
    keep = []
    for k in (1, 2):
        fh, ccs, disp, refs = parsed[k]
        for arch, hdr, nn, lat in ccs:
            dec.add(hdr, nn, lat, 0, 0)
    dec.run(); dec.wait()
    s = 0
    for k in (1, 2):
        fh, ccs, disp, refs = parsed[k]
        sets = []
        for arch, hdr, nn, lat in ccs:
            host = [dec.latent(s, g) for g in range(int(arch.n_grids))]
            dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in host]
            keep.append(dev)
            sets.append((arch, nn, [t.data_ptr() for t in dev]))
            enc.add(arch, nn, host)
            s += 1
        source = _frame_data(ic.case("vid3_ldp", k).src, int(fh.bitdepth), int(fh.frame_data_type))
        assert ev.add("P", sets[0], sets[1], [decoded[r] for r in refs], list(fh.global_flow), int(fh.warp_filter_size), source, owner=keep) == k - 1
    cands = ev.evaluate(lmbda, rate_deltas=True, distortion_deltas=True)
    enc.measure(); enc.wait()
    for f, (k, c) in enumerate(zip((1, 2), cands)):
        assert all(torch.equal(a, b) for a, b in zip(ev.planes(f), decoded[parsed[k][2]])), k
        r = [enc.rate(2 * f), enc.rate(2 * f + 1)]
        assert c.rates[0].total_bits == r[0].total_bits and c.rates[1].total_bits == r[1].total_bits
        assert c.bits == float(r[0].total_bits + r[1].total_bits) + 8.0 * float(r[0].n_bytes_nn + r[1].n_bytes_nn + r[0].n_bytes_header + r[1].n_bytes_header)
        n_samples, n_pixels = sum(c.quality.n), 128 * 224
        assert c.cost == c.mse + lmbda * c.bits / n_pixels
        for role in ("residue", "motion"):
            arch = parsed[k][1][ic.ROLES.index(role)][0]
            for g in range(int(arch.n_grids)):
                dd = torch.as_tensor(ev.distortion_delta_map(f, role, g), device="cuda").cpu().numpy()
                db = torch.as_tensor(ev.rate_delta_map(f, role, g), device="cuda").cpu().numpy().astype(np.float64)
                with np.errstate(invalid="ignore", over="ignore"):
                    want = dd.astype(np.float64) / (float(n_samples) * 255.0 * 255.0) + lmbda * db / float(n_pixels)
                    tol = 4.0 * 2.0 ** -52 * (np.abs(dd.astype(np.float64)) / (float(n_samples) * 255.0 * 255.0) + np.abs(lmbda * db / float(n_pixels)))
                none = (dd == SENTINEL) | np.isinf(db)
                got = ev.cost_delta_map(f, role, g, lmbda)
                assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == dd.shape
                got = got.cpu().numpy()
                # float64 on both sides, but not the same operations (the device may divide by a constant through its reciprocal):
                # the formula has four roundings, each at most half an ulp of one of its two terms
                assert np.array_equal(np.isposinf(got), none) and (np.abs(got - want)[~none] <= tol[~none]).all(), (k, role, g)
    ev.close(); enc.close(); dec.close()


@pytest.mark.gpu
def test_one_descent_step_per_role(gpu):
    """vid3_ldp frame 1 against the second set's reconstruction, grids (0, 1, 2): after a step of one role the frame's SSE is
    before + d_sse exactly, the bits within the rate deltas' bound of d_bits, and no latent of the frozen role has changed."""
    import torch

    import inter_cases as ic
    from cool_chic_amd import InterRdEvaluator

    case = ic.case("vid3_ldp", 1)
    lmbda = 1e-3
    dev = {r: case.cc[r].lat_dev.clone() for r in ic.ROLES}
    ev = InterRdEvaluator(0)
    ev.add(case.frame_type, *[(case.cc[r].arch, case.cc[r].nn, case.cc[r].ptrs(dev[r])) for r in ic.ROLES], case.refs, case.gflow, case.taps,
           _frame_data(case.src, case.bd, case.fdt), owner=dev)
    first, = ev.evaluate(lmbda)
    assert all(torch.equal(a, b) for a, b in zip(ev.planes(0), case.base_planes))
    # a cool-chic of another size than the frame is refused where the frame is known (the C call takes the size from the arch)
    from cool_chic_amd._lib import CCHeader
    small = CCHeader.from_buffer_copy(bytes(case.cc["motion"].arch))
    small.img_size[0] = 64
    with pytest.raises(ValueError, match="decodes to 64x224"):
        ev.add(case.frame_type, (case.cc["residue"].arch, case.cc["residue"].nn, case.cc["residue"].ptrs(dev["residue"])),
               (small, case.cc["motion"].nn, case.cc["motion"].ptrs(dev["motion"])), case.refs, case.gflow, case.taps,
               _frame_data(case.src, case.bd, case.fdt))
    assert len(ev) == 1
    for role in ic.ROLES:
        frozen = ic.ROLES[1 - ic.ROLES.index(role)]
        held = dev[frozen].clone()
        mine = dev[role].clone()
        (rep,), = ev.descend(lmbda, max_steps=1, grids=(0, 1, 2), roles=(role,))
        before, step = rep.before, rep.step
        assert rep.role == role
        i = ic.ROLES.index(role)
        bound, n = _step_bound(ev, 0, role, case.cc[role].arch, int(before.rates[i].n_symbols.sum()))
        # (a latent of the quarter-resolution motion cool-chic reaches far: its best candidate may block every other one)
        assert n == step.n_moves >= (2 if role == "residue" else 1) and step.n_candidates >= step.n_moves, (role, step)
        assert sum(step.n_moves_grid[3:]) == 0
        after, = ev.evaluate(lmbda)
        d_sse = sum(after.quality.sse) - sum(before.quality.sse)
        d_bits = (after.rates[0].total_bits - before.rates[0].total_bits) + (after.rates[1].total_bits - before.rates[1].total_bits)
        print(f"vid3_ldp[1] {role}: {step.n_candidates} candidates, {step.n_moves} moves, d_sse {d_sse} (step {step.d_sse}), d_bits {d_bits!r} "
              f"(step {step.d_bits!r}, |diff| {abs(d_bits - step.d_bits):.3g}, bound {bound:.3g}), cost {before.cost!r} -> {after.cost!r}")
        assert d_sse == step.d_sse
        assert abs(d_bits - step.d_bits) <= bound
        assert after.rates[1 - i].total_bits == before.rates[1 - i].total_bits
        assert step.d_cost < 0 and after.cost < before.cost
        assert torch.equal(dev[frozen], held) and not torch.equal(dev[role], mine)
        assert int((dev[role] != mine).sum()) == step.n_moves
    # descend() alternates the roles and stops when a full cycle moved nothing
    reports = ev.descend(lmbda, max_steps=2, grids={"residue": (0, 1), "motion": (0,)})
    assert [r[0].role for r in reports] == ["residue", "motion"]
    assert len(ev.descend(lmbda, max_steps=5, min_gain=1e9)) == 2  # nothing can move: one idle cycle
    ev.close()


@pytest.mark.gpu
def test_requantise_video_tool(gpu, tmp_path):
    """tools/requantise_video.py on vid3_ldp against a .yuv of the second sets' reconstructions, --max-steps 2 --grids 0,1,2: exit
    status 0 (its own decode-back assertion inside), the output parses, and decodes to per-frame costs that sum to no more than the
    input's."""
    import subprocess
    import sys

    import torch

    import inter_cases as ic
    from conftest import GOLDEN
    from cool_chic_amd import DecodeBatch
    from cool_chic_amd.bitstream.decode import _split_frame, decode_video
    from cool_chic_amd.bitstream.header import VideoHeader

    lmbda = 1e-3
    parsed = ic.parse_video("vid3_ldp")
    # frame 0: the intra cool-chic under its second latent set; frames 1 and 2: the cases' sources
    fh, ((arch, hdr, nn, lat),), _, _ = parsed[0]
    dec = DecodeBatch(0)
    dec.add(hdr, nn, lat, 8, 1)
    dec.run(); dec.wait()
    rng = np.random.default_rng(5)
    lat2 = [np.clip(dec.latent(0, g).astype(np.int16) + rng.integers(-2, 3, size=(arch.grid_h[g], arch.grid_w[g])), -64, 63).astype(np.int8)
            for g in range(int(arch.n_grids))]
    dec.add_latents(arch, nn, lat2, 8, 1)
    dec.run(); dec.wait()
    sources = [dec.planes(1)] + [[p.cpu().numpy() for p in ic.case("vid3_ldp", k).src] for k in (1, 2)]
    dec.close()
    yuv, out = str(tmp_path / "source.yuv"), str(tmp_path / "out.cool")
    with open(yuv, "wb") as f:
        for planes in sources:
            for p in planes:
                f.write(np.ascontiguousarray(p, dtype=np.uint8).tobytes())
    torch.cuda.synchronize()
    src = os.path.join(GOLDEN, "vid3_ldp.cool")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "requantise_video.py"), src, yuv, out, "--lmbda", str(lmbda),
                          "--max-steps", "2", "--grids", "0,1,2"], cwd=ROOT, capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stderr[-2000:]
    assert "before:" in run.stdout and "after:" in run.stdout

    def costs(path):
        with open(path, "rb") as f:
            rest = VideoHeader().read_header(f.read())   # ccd_read_video_header
        frames = decode_video(path)
        total = []
        for k in range(3):                               # vid3_ldp: coding order = display order
            n0 = len(rest)
            fh, ccs, rest = _split_frame(rest)           # ccd_read_frame_header, ccd_read_cc_header
            assert len(ccs) == (1 if k == 0 else 2)
            planes = frames[str(k)].integer_planes()
            sse = sum(int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum()) for a, b in zip(planes, sources[k]))
            n = sum(a.size for a in planes)
            total.append(sse / (n * 255.0 * 255.0) + lmbda * 8.0 * (n0 - len(rest)) / (128 * 224))
        assert rest == b""
        return total

    before, after = costs(src), costs(out)
    print("cost per frame before", before, "after", after)
    assert sum(after) <= sum(before)
