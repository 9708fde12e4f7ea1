"""Every instantiation of the fused float kernel (ccd_fused_kernel.inc::decode_fused_kernel<CIN, C, MODE, NZ>, DESIGN.md section
4.2) against the CPU oracle, f32 bit for bit: 5 .. 9 latent levels x 2 .. 5 output channels in the three forms of the float path
(CCD_OPT_FUSED_DEC = 2: kFdPre behind the kFdPyr launch, 1: kFdWhole, 0: unfused), common randomness (NZ = CIN) at every level
count, at dense-grid sizes around the 64 x 32 tile and the run of 8 tiles (tests/float_matrix.py makes the cases).

Bars: latents == what was encoded; `output` == the oracle's `out` and (unfused) `dense` == the oracle's `dense` as uint32 words,
no tolerance; integer planes of the three-channel cases == oracle.decode_video; the kernel that served a slot is asserted from
ccd_batch_slot_kernels, never assumed - a pair that fell back to the unfused path would otherwise pass unnoticed."""
import numpy as np
import pytest

import float_matrix as fm
from conftest import load_golden

PAIRS = [(n, c) for n in fm.LEVELS for c in fm.CHANNELS]
# (levels, C) -> fused_dec_lds_bytes, for pairs whose fused kernel would need more than the 160 KB of LDS the plan allows
# (ccd_batch_plan.cpp: layout_fused_dec) and which therefore run the unfused path with CCD_OPT_FUSED_DEC = 1 / 2.  None does:
# fd_layout + the parameter block give at most 80 864 bytes (9 levels, 5 channels, one-launch form, taken with 64 hidden units and
# three 3x3 layers), 61 120 behind the pyramid launch - half the cap.  A pair that lands here keeps every output comparison.
OVER_LDS_CAP = {}


# ---- CPU -------------------------------------------------------------------------------------------------------------
def test_inventory_covers_every_instantiation(oracle):
    """The inventory: every case splits, parses and decodes in the oracle to the latents that were encoded and to a finite output
    that is not constant in any channel, with a network inside the finite envelope (the matrix-core kernel is eligible); over all
    cases the (levels, C) pairs are exactly 5 .. 9 x 2 .. 5 at every common size, and common randomness covers 5 .. 9 levels."""
    from cool_chic_amd._lib import lib

    cases = fm.cases(load_golden, oracle)
    assert len({c.label for c in cases}) == len(cases)
    for c in cases:
        hdr, nn, lat = c.triple
        assert fm.EXPECTED_C.get((c.donor, c.cc), 3) == c.c, c.label
        h, geo = oracle.read_cc_header(hdr)
        assert (h.nn_n_bytes, h.n_bytes_latent) == (len(nn), len(lat)), c.label
        levels = [g for g in range(geo.n_grids) if not geo.is_hyper[g]]
        assert len(levels) == c.levels and (geo.grid_h[levels[0]], geo.grid_w[levels[0]]) == c.dense, c.label
        assert geo.input_feature_synthesis == c.levels * (2 if c.cr else 1), c.label
        if c.picture:
            (fh, ccs), = oracle.split_stream(c.stream)[1]
            assert ccs == [c.triple] and (fh.bitdepth, fh.frame_data_type) == (c.bitdepth, c.frame_data_type), c.label
        ref = fm.reference(oracle, c)
        assert ref["n_grids"] == len(c.latents), c.label
        for g, a in enumerate(c.latents):
            assert np.array_equal(ref["latent"][g], a), f"{c.label}: the oracle decodes other latents in grid {g}"
        assert {int(a.min()) for a in c.latents} >= {-64} and {int(a.max()) for a in c.latents} >= {63}, c.label
        out = ref["out"]
        assert out.shape[0] == c.c and ref["dense"].shape[1:] == c.dense, c.label
        assert np.isfinite(out).all(), c.label
        for ch in range(c.c):
            assert np.unique(out[ch]).size >= 2, f"{c.label}: channel {ch} is constant"
        assert lib().ccd_network_kernel_class(hdr, len(hdr), nn, len(nn)) & 128 == 0, f"{c.label}: outside the finite envelope"
    for size in fm.SIZES:
        assert {(c.levels, c.c) for c in cases if c.dense == size and not c.cr} == set(PAIRS), size
        assert {c.levels for c in cases if c.dense == size and c.cr} == set(fm.LEVELS), size
    assert {(c.levels, c.c) for c in cases} == set(PAIRS)
    assert {(c.levels, c.c) for c in cases if c.dense == fm.LARGE and not c.cr} == {(n, ch) for n in fm.LARGE_LEVELS for ch in fm.CHANNELS}
    assert {c.levels for c in cases if c.dense == fm.LARGE and c.cr} == set(fm.LARGE_LEVELS)
    assert {(c.donor, c.levels, c.bitdepth, c.frame_data_type) for c in cases if c.donor.startswith("yuv")} == \
        {("yuv420_8b", 5, 8, 1), ("yuv420_8b", 9, 8, 1), ("yuv444_10b", 6, 10, 2), ("yuv444_10b", 8, 10, 2)}
    for (n, ch) in PAIRS:
        assert len(_alone_case(cases, n, ch)) == 1


def test_comparison_reports_a_single_ulp():
    """The comparison is on the words: one element moved by one ulp (or from 0.0 to -0.0) is a difference, reported with its
    index; equal arrays are None; the message names what the person fixing it needs."""
    rng = np.random.default_rng(5)
    a = rng.standard_normal((3, 33, 65)).astype(np.float32)
    assert fm.first_difference(a, a.copy()) is None
    b = a.copy()
    b[2, 32, 64] = np.nextafter(b[2, 32, 64], np.float32(np.inf))
    assert fm.first_difference(b, a) == ((2, 32, 64), 1)
    b[1, 7, 0] = np.nextafter(b[1, 7, 0], np.float32(-np.inf))
    assert fm.first_difference(b, a) == ((1, 7, 0), 2)
    z = np.zeros((2, 4, 4), np.float32)
    m = z.copy()
    m[0, 3, 1] = -0.0
    assert np.array_equal(m, z) and fm.first_difference(m, z) == ((0, 3, 1), 1)
    p = np.arange(12, dtype=np.uint16).reshape(3, 4)
    q = p.copy()
    q[1, 2] += 1
    assert fm.first_difference(q, p) == ((1, 2), 1)
    with pytest.raises(AssertionError):
        fm.first_difference(a[:, :32], a)
    case = fm.Case("rgb192.cc0 n=8 dense=33x65", "rgb192", 0, 8, (33, 65), 3, False, True, 8, 0, None, None, None, None)
    msg = fm.describe(case, 2, "output", b, a)
    for word in ("rgb192.cc0", "n=8", "33x65", "fused_dec=2", "output", "channel 1", "(row, column) = (7, 0)", "2 of 6435"):
        assert word in msg, (word, msg)
    assert fm.describe(case, 2, "output", a, a.copy()) is None


# ---- GPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cool_chic_amd import DecodeBatch, _lib

    _lib.lib()
    return DecodeBatch


def _alone_case(cases, n, ch):
    name, k = fm.ALONE_DONORS[ch]
    return [i for i, c in enumerate(cases) if (c.donor, c.cc, c.levels, c.dense, c.c) == (name, k, n, (33, 65), ch)]


def _read(b, slot, case):
    k = b.slot_kernels(slot)
    return {"status": b.slot_status(slot), "kernels": k, "latent": [b.latent(slot, g) for g in range(len(case.latents))],
            "output": b.output(slot), "dense": None if k & 4 else b.dense(slot), "planes": b.planes(slot) if case.picture else None}


_BATCH = {}


def _decoded(gpu, oracle, form):
    """ALL cases in ONE batch with CCD_OPT_FUSED_DEC = form, one run: every level count and channel count at once, so that the
    launch tables (the pyramid groups, the (levels, channels) frame groups) hold several groups each.  Once per process; a batch
    that failed is not run again."""
    if form not in _BATCH:
        cases = fm.cases(load_golden, oracle)
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
    """(bit 2: the fused float kernel, bit 6: its form behind the pyramid launch) a slot must report."""
    if form == 0 or (case.levels, case.c) in OVER_LDS_CAP:
        return False, False
    if case.cr and form == 1:  # the one-launch form has no common-randomness instantiation: such a stream runs unfused
        return False, False
    return True, form == 2


@pytest.mark.gpu
@pytest.mark.parametrize("form", [2, 1, 0])
def test_every_instantiation_matches_the_oracle(gpu, oracle, form):
    """form 2: decode_fused_kernel<CIN, C, kFdPre, NZ> behind the kFdPyr launch (the default); 1: <CIN, C, kFdWhole>; 0: the
    unfused kernels, which also expose the dense stack."""
    cases = fm.cases(load_golden, oracle)
    got = _decoded(gpu, oracle, form)
    bad = []
    for c, r in zip(cases, got):
        ref = fm.reference(oracle, c)
        k = r["kernels"]
        if r["status"] != 0:
            bad.append(f"{c.label} fused_dec={form}: slot status {r['status']}")
        fused, pre = _expected_fused(c, form)
        if (bool(k & 4), bool(k & 64)) != (fused, pre) or k & 128 or (form == 0 and k & 8):
            bad.append(f"{c.label} C={c.c} fused_dec={form}: slot_kernels {k:#x}, expected bit 2 {fused}, bit 6 {pre}, bits 3 (unfused) and 7 clear")
        for g, a in enumerate(c.latents):
            if not np.array_equal(r["latent"][g], a):
                bad.append(f"{c.label} fused_dec={form}: latent grid {g} differs from what was encoded")
        bad.append(fm.describe(c, form, "synthesis output", r["output"], ref["out"]))
        if not fused:
            assert r["dense"] is not None
            bad.append(fm.describe(c, form, "dense stack (Upsampling.forward)", r["dense"], ref["dense"]))
        if c.picture:
            for p, (a, w) in enumerate(zip(r["planes"], fm.reference_planes(oracle, c))):
                bad.append(fm.describe(c, form, f"integer plane {p}", a.astype(np.uint16), w))
    bad = [m for m in bad if m]
    assert not bad, f"{len(bad)} failures, the first of them:\n" + "\n".join(bad[:12])


@pytest.mark.gpu
@pytest.mark.parametrize("n,ch", PAIRS)
def test_alone_equals_the_big_batch(gpu, oracle, n, ch):
    """One cool-chic of the pair at 33 x 65 ALONE in a batch (default form): the words it gave among the 134 of the big batch -
    a result does not depend on which groups share the launch tables."""
    cases = fm.cases(load_golden, oracle)
    (i,) = _alone_case(cases, n, ch)
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
    bad = [fm.describe(c, "2 alone", "synthesis output", r["output"], want["output"], "in the big batch")]
    if c.picture:
        bad += [fm.describe(c, "2 alone", f"integer plane {p}", a, w, "in the big batch") for p, (a, w) in enumerate(zip(r["planes"], want["planes"]))]
    bad = [m for m in bad if m]
    assert not bad, "\n".join(bad)
