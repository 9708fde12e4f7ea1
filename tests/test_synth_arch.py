"""Synthesis and upsampling shapes the reference-encoded fixtures never have (tests/synth_arch.py makes the cases): the fused
synthesis kernel (ccd_synth_fused.hip::syn_fused_kernel<CP, C>), the generic per-layer kernel (ccd_float.hip::syn_layer_kernel) and
both branches of upsample_generic_one, each reached by a network's OWN shape, and ccd_latent_footprint for those shapes.

The oracle's loops for these shapes (cc_oracle.c::tconv_up2, preconv, syn_conv) have the structure of the device's generic code
and are pinned to the reference decoder only at the fixtures' sizes, so the oracle is first held against a float64 statement of
the float path written from the operations the reference calls (tests/synth_arch_ref.py), under a bar measured per case and
stage; then the device is held against the oracle word for word.

Bars on the GPU: status 0; latents == what was encoded; `output` == the oracle's `out` and (unfused) `dense` == the oracle's
`dense` as uint32 words, no tolerance; integer planes of the picture cases == oracle.decode_video; ccd_batch_slot_kernels & 2
(fused synthesis kernel) and & 4 (fused float kernel) as tests/synth_arch.py STATES them per architecture - a case that silently
changed path fails.

Measured on the CPU (printed by the tests): the oracle reaches at most 0.54 of the float64 bar (ups14x15 dense=7x9, both
stages)."""
import numpy as np
import pytest

import float_matrix as fm
import synth_arch as sa
import synth_arch_ref as sr
from conftest import GOLDEN, load_golden

FORMS = [2, 1, 0]
# what of synth_arch.ALL_FACTS some header of the rest of the suite (the fixtures, float_matrix, float_tail, float_classes) has: the
# common-randomness cases of float_matrix at 7 and 8 levels have 14 and 16 dense channels and run the fused synthesis kernel with
# CCD_OPT_FUSED_DEC = 0 / 1.  Everything else in ALL_FACTS is new with tests/synth_arch.py.
REACHED_BEFORE = {"CP 16"}


# ---- CPU -------------------------------------------------------------------------------------------------------------
def _headers_of_the_rest_of_the_suite(oracle):
    import glob
    import os

    import float_classes
    import float_tail as ft
    from cool_chic_amd import writer

    hdrs = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "*.cool"))):
        with open(path, "rb") as f:
            hdrs += [cc[0] for _fh, ccs in oracle.split_stream(f.read())[1] for cc in ccs]
    hdrs += [c.triple[0] for c in fm.cases(load_golden, oracle)]
    hdrs += [c.triple[0] for c in ft.cases(load_golden, oracle)]
    hdrs += [triple[0] for triple, _stream, _fin in float_classes.crafted(load_golden, oracle).values()]
    return [writer.parse_cc_header(h) for h in hdrs]


def test_inventory_covers_the_matrix(oracle):
    """Every case splits, parses and decodes in the oracle to the latents that were encoded and to a finite output that is not
    constant in any channel, with an NN payload the header can name; the rows of synth_arch.ARCHS cover exactly the lines of the
    matrix, every row at every common size; each row has the shape its lines name (kernel sizes, halo, channel padding, flags);
    and of those shapes the rest of the suite - fixtures, float_matrix, float_tail, float_classes - reaches REACHED_BEFORE only."""
    from cool_chic_amd import writer
    from cool_chic_amd._lib import lib

    cases = sa.cases(load_golden, oracle)
    assert len({c.label for c in cases}) == len(cases)
    largest = 0
    for c in cases:
        hdr, nn, lat = c.triple
        assert sa.EXPECTED_C.get((c.donor, c.cc)) == c.c or c.spec.fmt == "float", c.label
        h, geo = oracle.read_cc_header(hdr)
        assert (h.nn_n_bytes, h.n_bytes_latent) == (len(nn), len(lat)), c.label
        assert 0 < len(nn) <= writer.MAX_NN_BYTES, c.label
        largest = max(largest, len(nn))
        levels = [g for g in range(geo.n_grids) if not geo.is_hyper[g]]
        assert len(levels) == c.levels and (geo.grid_h[levels[0]], geo.grid_w[levels[0]]) == c.dense, c.label
        assert geo.input_feature_synthesis == c.levels * (2 if c.cr else 1), c.label
        parsed = writer.parse_cc_header(hdr)
        assert (parsed.ups_k_size, parsed.ups_preconcat_k_size) == c.spec.ups, c.label
        if c.spec.layers is not None:
            assert [(l.out_ft, l.k_size, l.mode, l.non_linearity) for l in parsed.syn_layer[:parsed.n_layer_synthesis]] == list(c.spec.layers), c.label
        if c.picture:
            (fh, ccs), = oracle.split_stream(c.stream)[1]
            assert ccs == [c.triple] and (fh.bitdepth, fh.frame_data_type) == (c.bitdepth, c.frame_data_type), c.label
        else:
            assert c.bitdepth == 0 and c.stream is None, c.label
        ref = sa.reference(oracle, c)
        assert ref["n_grids"] == len(c.latents), c.label
        for g, a in enumerate(c.latents):
            assert np.array_equal(ref["latent"][g], a), f"{c.label}: the oracle decodes other latents in grid {g}"
        assert {int(a.min()) for a in c.latents} >= {-64} and {int(a.max()) for a in c.latents} >= {63}, c.label
        out = ref["out"]
        assert out.shape[0] == c.c and ref["dense"].shape[1:] == c.dense and ref["syn_out"].shape[1:] == c.dense, c.label
        assert np.isfinite(out).all() and np.isfinite(ref["dense"]).all(), c.label
        for ch in range(c.c):
            assert np.unique(out[ch]).size >= 2, f"{c.label}: channel {ch} is constant"
        # inside the finite envelope: a case the table sends to the fused float kernel is not kept from it by its values
        assert lib().ccd_network_kernel_class(hdr, len(hdr), nn, len(nn)) & 128 == 0, f"{c.label}: outside the finite envelope"
    print(f"{len(cases)} cases of {len(sa.ARCHS)} architectures, largest NN payload {largest} bytes of {writer.MAX_NN_BYTES}")

    # ---- the set ----
    assert len({s.name for s in sa.ARCHS}) == len(sa.ARCHS)
    assert set().union(*(s.lines for s in sa.ARCHS)) == sa.MATRIX
    for s in sa.ARCHS:
        want = (sa.SIZES_420 if s.donor == sa.YUV420 else sa.SIZES) + ([sa.HALO9_SIZE] if "halo9" in s.lines else [])
        assert [c.dense for c in cases if c.arch_name == s.name] == want, s.name
    assert set(sa.ALONE) <= {s.name for s in sa.ARCHS}
    by = {}
    for c in cases:
        by.setdefault(c.arch_name, c)

    def shape(name):
        a = by[name].arch
        L = [a.syn_layer[i] for i in range(a.n_layer_synthesis)]
        return a, L, sum((l.k_size - 1) // 2 for l in L[2:]), sa.facts(a)

    def fused_shape(L, c):  # what ccd_batch_plan.cpp::layout_synthesis asks of the layers
        return (2 <= len(L) <= 5 and all(l.k_size == 1 and l.mode == sa.LIN for l in L[:2]) and L[1].out_ft == c
                and all(l.out_ft == c and l.k_size <= 7 for l in L[2:]))

    for s in sa.ARCHS:
        a, L, halo, f = shape(s.name)
        n_dense = a.input_feature_synthesis
        assert (s.syn == "fused") == (fused_shape(L, a.out_channels) and 2 <= a.out_channels <= 5 and n_dense <= 16 and halo <= 11), s.name
        levels = by[s.name].levels
        fdec = (5 <= levels <= 9 and 2 <= a.out_channels <= 5 and s.ups == (8, 7) and fused_shape(L, a.out_channels)
                and all(l.k_size == 3 for l in L[2:]))
        assert s.fdec == fdec, s.name
    _, L, halo, f = shape("k5k7")
    assert [l.k_size for l in L[2:]] == [5, 7] and halo == 5 and {"conv k=5", "conv k=7", "conv linear"} <= f
    _, L, halo, f = shape("halo9")
    assert halo == 9 and "n_conv 3" in f and 32 - 2 * halo == sa.HALO9_SIZE[0] - 1 and 64 - 2 * halo == sa.HALO9_SIZE[1] - 1
    _, L, halo, f = shape("nconv3")
    assert [(l.k_size, l.mode) for l in L[2:]] == [(3, sa.LIN), (3, sa.RES), (3, sa.LIN)] and "n_conv 3" in f
    assert "conv k=1" in shape("k1conv")[3]
    a, L, _, _ = shape("two1x1")
    assert len(L) == 2 and (L[0].non_linearity, L[1].non_linearity) == (sa.NONE, sa.RELU)
    assert shape("hidden1")[1][0].out_ft == 1 and shape("hidden127")[1][0].out_ft == 127
    assert "no stabiliser" in shape("nostab")[3] and "no stabiliser" not in shape("stab")[3]
    assert [shape(n)[0].out_channels for n in ("c2", "k5k7", "c4", "c5")] == [2, 3, 4, 5]
    assert [by[n].levels for n in ("lv1", "lv2", "lv4")] == [1, 2, 4] and all("CP 4" in shape(n)[3] for n in ("lv1", "lv2", "lv4"))
    assert [shape(n)[0].input_feature_synthesis for n in ("cr7", "cr8", "cr9")] == [14, 16, 18] and all(by[n].cr for n in ("cr7", "cr8", "cr9"))
    assert "CP 16" in shape("cr7")[3] and "CP 16" in shape("cr8")[3]
    assert len(shape("one")[1]) == 1 and shape("first3")[1][0].k_size == 3 and shape("l1wide")[1][1].out_ft != 3
    a, L, _, _ = shape("seven")
    assert len(L) == 7 and L[-1].k_size == 9 and any(l.k_size > 1 and l.out_ft != p.out_ft for p, l in zip(L[1:], L[2:]))
    assert shape("k15")[1][-1].k_size == 15 and min(sa.SIZES) == (7, 9)  # 7 x 9: most of the 15 x 15 taps of every window are clamped
    assert shape("out1")[0].out_channels == 1 and shape("out6")[0].out_channels == 6 and not by["out1"].picture and not by["out6"].picture
    assert {(by[n].bitdepth, by[n].frame_data_type) for n in ("k5k7", "p420", "p444")} == {(8, 0), (8, 1), (10, 2)}
    assert all({"conv k=5", "conv k=7"} <= shape(n)[3] for n in ("p420", "p444"))
    for u, p in sa.UPS_PAIRS:
        for tail, n in (("", 7), ("lv2", 2)):
            c = by[f"ups{u}x{p}{tail}"]
            assert (c.arch.ups_k_size, c.arch.ups_preconcat_k_size, c.levels) == (u, p, n)
    new = set().union(*(sa.facts(c.arch) for c in cases))
    assert new == sa.ALL_FACTS, sa.ALL_FACTS - new

    # ---- the rest of the suite ----
    before = set().union(*(sa.facts(h) for h in _headers_of_the_rest_of_the_suite(oracle)))
    print("of", sorted(sa.ALL_FACTS), "the rest of the suite has", sorted(before))
    assert before == REACHED_BEFORE


_STAGES = {}


def _stages(oracle, c):
    if c.label not in _STAGES:
        ref = sa.reference(oracle, c)
        _STAGES[c.label] = sr.float_path(c.arch, c.triple[1], c.latents, ref["dense"][c.levels:] if c.cr else None)
    return _STAGES[c.label]


def test_oracle_against_float64(oracle):
    """Per case and stage (`dense`: the latent channels of the dense stack; `syn_out`: the synthesis output): the oracle's distance
    from the float64 statement of the float path stays under 2 x (a torch float32 run's distance) + 8 units of 2^-23 max|ref64|
    (tests/synth_arch_ref.py).  No case is left out.  Prints the largest fraction of the bar reached per stage."""
    cases = sa.cases(load_golden, oracle)
    worst, bad, n = {"dense": (0.0, None), "syn_out": (0.0, None)}, [], 0
    for c in cases:
        ref = sa.reference(oracle, c)
        st = _stages(oracle, c)
        for stage, got in (("dense", ref["dense"][:c.levels]), ("syn_out", ref["syn_out"])):
            ref64, run32 = st[stage]
            assert got.shape == ref64.shape and np.isfinite(ref64).all(), (c.label, stage)
            bar, measured = sr.bar(ref64, run32)
            err = np.abs(got.astype(np.float64) - ref64)
            d = float(err.max())
            n += 1
            if d / bar > worst[stage][0]:
                worst[stage] = (d / bar, c.label)
            if not d <= bar:
                idx = tuple(int(i) for i in np.unravel_index(int(err.argmax()), err.shape))
                bad.append(f"{c.label} {stage}: |oracle - ref64| {d:.3e} at {idx} over the bar {bar:.3e} (float32 run {measured:.3e}, max|ref64| {np.abs(ref64).max():.3e})")
    print(f"{n} comparisons; largest fraction of the bar: " + ", ".join(f"{s} {w:.3f} ({l})" for s, (w, l) in worst.items()))
    assert n == 2 * len(cases)
    assert not bad, f"{len(bad)} over the bar, the first of them:\n" + "\n".join(bad[:8])


def test_footprint_by_impulse_in_the_oracle(oracle):
    """ccd_latent_footprint for other filter and layer sizes than 8 / 7 / 3 x 3 (test_float_tail.py has those): per shape of
    synth_arch.FOOTPRINT_ARCHS and the motion donor (nearest final resize) at two picture sizes, in every latent grid one latent
    flipped between the ends of the alphabet at the four corners, the centre and three seeded positions, re-encoded and decoded
    by the oracle: no output word outside the clipped box changes, and per shape every side of the box is tight (slack 0) for
    some flip."""
    from test_distortion_deltas import _box_of

    from cool_chic_amd import writer
    from cool_chic_amd.dsens import latent_footprint

    def decode(arch, nn, lat):
        blob = writer.encode_coolchic(arch, nn, lat)
        h = writer.parse_cc_header(blob)
        a, b = h.n_bytes_header, h.n_bytes_header + h.nn_n_bytes
        return oracle.decode_coolchic(blob[:a], blob[a:b], blob[b:])["out"].view(np.uint32)

    specs = [s for s in sa.ARCHS if s.name in sa.FOOTPRINT_ARCHS] + [sa.FOOTPRINT_MOTION]
    assert len(specs) == len(sa.FOOTPRINT_ARCHS) + 1
    rng = np.random.default_rng(20261020)
    total = 0
    for spec in specs:
        n_flips, slack, inner = 0, [None] * 4, [None] * 4
        for size in sa.FOOTPRINT_SIZES:
            label, arch, nn, latents = sa.footprint_case(load_golden, oracle, spec, size)
            H, W = size
            base = decode(arch, nn, latents)
            assert base.shape[1:] == (H, W), label
            for g in range(arch.n_grids):
                if arch.is_hyperlatent[g]:
                    continue
                h, w = latents[g].shape
                pos = {(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2)}
                pos |= {(int(rng.integers(h)), int(rng.integers(w))) for _ in range(3)}
                box = latent_footprint(arch, g)
                for y, x in sorted(pos):
                    l2 = list(latents)
                    l2[g] = latents[g].copy()
                    l2[g][y, x] = 63 if l2[g][y, x] < 0 else -64
                    diff = (decode(arch, nn, l2) != base).any(axis=0)
                    n_flips += 1
                    y0, x0, y1, x1 = _box_of(arch, g, y, x, box)
                    rows, cols = np.flatnonzero(diff.any(axis=1)), np.flatnonzero(diff.any(axis=0))
                    assert rows.size, (label, g, y, x)
                    found = (rows[0], cols[0], rows[-1], cols[-1])
                    assert found[0] >= y0 and found[1] >= x0 and found[2] <= y1 and found[3] <= x1, \
                        (label, g, y, x, "changed", found, "box", (y0, x0, y1, x1))
                    sides = [(y0 > 0, found[0] - y0), (x0 > 0, found[1] - x0), (y1 < H - 1, y1 - found[2]), (x1 < W - 1, x1 - found[3])]
                    for k, (free, s) in enumerate(sides):
                        slack[k] = int(s) if slack[k] is None else min(slack[k], int(s))
                        if free:
                            inner[k] = int(s) if inner[k] is None else min(inner[k], int(s))
        print(f"{spec.name} ups {spec.ups}: {n_flips} flips, smallest slack (top, left, bottom, right) {slack}; on the sides the picture does not clip {inner}")
        assert n_flips >= 42, spec.name
        assert slack == [0, 0, 0, 0], spec.name
        if spec is not sa.FOOTPRINT_MOTION:  # no final resize: the box adds no margin, it is exact where the picture does not clip it
            assert inner == [0, 0, 0, 0], spec.name
        total += n_flips
    print(f"{total} flips in all")


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
            "output": b.output(slot), "dense": None if k & 4 else b.dense(slot), "planes": b.planes(slot) if case.picture else None}


_BATCH = {}


def _decoded(gpu, oracle, form, forced_generic=False):
    """ALL cases in ONE batch with CCD_OPT_FUSED_DEC = form, run twice: (the first run's results, the second's).  Once per process
    and key; a batch that failed is not run again.  `forced_generic`: the caller has set CCD_FORCE_GENERIC for the batch."""
    key = (form, forced_generic)
    if key not in _BATCH:
        cases = sa.cases(load_golden, oracle)
        try:
            b = gpu(0, fused_dec=form)
            try:
                for c in cases:
                    b.add(*c.triple, c.bitdepth, c.frame_data_type)
                runs = []
                for _ in range(2):
                    b.run()
                    b.wait()
                    runs.append([_read(b, i, c) for i, c in enumerate(cases)])
                _BATCH[key] = tuple(runs)
            finally:
                b.close()
        except Exception as e:
            _BATCH[key] = e
    if isinstance(_BATCH[key], Exception):
        raise _BATCH[key]
    return _BATCH[key]


def _check(oracle, cases, got, form, forced_generic):
    bad = []
    how = "generic forced" if forced_generic else form
    for c, r in zip(cases, got):
        ref = sa.reference(oracle, c)
        k = r["kernels"]
        if r["status"] != 0:
            bad.append(f"{c.label} fused_dec={how}: slot status {r['status']}")
        syn, fdec = sa.expected_kernels(c, form, forced_generic)
        if (bool(k & 2), bool(k & 4)) != (syn, fdec) or k & 128 or (forced_generic and k & 1):
            bad.append(f"{c.label} C={c.c} fused_dec={how}: slot_kernels {k:#x}, the case table says & 2 (fused synthesis kernel) {syn}, & 4 (fused float kernel) {fdec}, & 128 clear")
        for g, a in enumerate(c.latents):
            if not np.array_equal(r["latent"][g], a):
                bad.append(f"{c.label} fused_dec={how}: latent grid {g} differs from what was encoded")
        bad.append(fm.describe(c, how, "output", r["output"], ref["out"]))
        if not k & 4:
            assert r["dense"] is not None
            bad.append(fm.describe(c, how, "dense stack (Upsampling.forward)", r["dense"], ref["dense"]))
        if c.picture:
            for p, (a, w) in enumerate(zip(r["planes"], sa.reference_planes(oracle, c))):
                bad.append(fm.describe(c, how, f"integer plane {p}", a.astype(np.uint16), w))
    return [m for m in bad if m]


def _same(c, r, want, how, yardstick):
    bad = []
    if (r["status"], r["kernels"]) != (want["status"], want["kernels"]):
        bad.append(f"{c.label} {how}: status / slot_kernels {r['status']} {r['kernels']:#x}, {yardstick} {want['status']} {want['kernels']:#x}")
    bad.append(fm.describe(c, how, "output", r["output"], want["output"], yardstick))
    if r["dense"] is not None and want["dense"] is not None:
        bad.append(fm.describe(c, how, "dense stack", r["dense"], want["dense"], yardstick))
    if c.picture:
        bad += [fm.describe(c, how, f"integer plane {p}", a, w, yardstick) for p, (a, w) in enumerate(zip(r["planes"], want["planes"]))]
    return [m for m in bad if m]


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_every_architecture_matches_the_oracle(gpu, oracle, form):
    """All cases in one batch per form of the float path (2: the default, 1: the one-launch fused float kernel, 0: unfused, which
    also exposes the dense stack of every slot); the second run of the batch gives the words of the first."""
    cases = sa.cases(load_golden, oracle)
    first, second = _decoded(gpu, oracle, form)
    bad = _check(oracle, cases, first, form, False)
    for c, r, w in zip(cases, second, first):
        bad += _same(c, r, w, f"fused_dec={form} second run", "in the first run")
    assert not bad, f"{len(bad)} failures, the first of them:\n" + "\n".join(bad[:12])


@pytest.mark.gpu
def test_every_architecture_through_the_generic_kernels(gpu, oracle, monkeypatch):
    """The same batch with CCD_FORCE_GENERIC (as test_gpu_parity.py::test_generic_fallback_kernels sets it): every architecture
    through syn_layer_kernel and the unfused pyramid, against the same oracle words."""
    monkeypatch.setenv("CCD_FORCE_GENERIC", "1")
    cases = sa.cases(load_golden, oracle)
    first, second = _decoded(gpu, oracle, 2, forced_generic=True)
    bad = _check(oracle, cases, first, 2, True)
    for c, r, w in zip(cases, second, first):
        bad += _same(c, r, w, "generic forced, second run", "in the first run")
    assert not bad, f"{len(bad)} failures, the first of them:\n" + "\n".join(bad[:12])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sa.ALONE)
def test_alone_equals_the_big_batch(gpu, oracle, name):
    """One case per architecture class ALONE in a batch (default form): the words it gave in the big batch - a result does not
    depend on which frames share the launch tables of the pyramid steps and of the fused synthesis kernel."""
    cases = sa.cases(load_golden, oracle)
    i = next(i for i, c in enumerate(cases) if c.arch_name == name)
    c, want = cases[i], _decoded(gpu, oracle, 2)[0][i]
    b = gpu(0, fused_dec=2)
    try:
        b.add(*c.triple, c.bitdepth, c.frame_data_type)
        b.run()
        b.wait()
        r = _read(b, 0, c)
    finally:
        b.close()
    assert r["status"] == 0, (c.label, r["status"])
    bad = _same(c, r, want, "2 alone", "in the big batch")
    assert not bad, "\n".join(bad)
