"""Distortion deltas (ccd_dsens_*, ccd_latent_footprint, DistortionDeltas, RdEvaluator.cost_delta_map):
for every latent the exact change of the frame's squared error if that one latent were v - 1 or v + 1.

The reference is brute force from code other test files pin: the latents with ONE value moved on the host go through given-latent
slots of a DecodeBatch (64 candidates per run) and QualityMeter.score_planes gives the exact integer SSE of each; the reference
entry is SSE(moved) - SSE(base).  Everything is compared as integers, no tolerance.  The source of a case is what a DIFFERENT
random latent set decodes to, so the deltas take both signs; the latents are random in [-12, 12] (the full alphabet saturates
the planes and would make most deltas zero) with some forced to -64 and 63."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT, load_golden

ERR_VALUE, ERR_ARG = -2, -7
SENTINEL = -2 ** 63
ENTRY_POINTS = ["ccd_latent_footprint", "ccd_latent_probe_stride", "ccd_dsens_create", "ccd_dsens_destroy", "ccd_dsens_add", "ccd_dsens_run",
                "ccd_dsens_wait", "ccd_dsens_slot_map", "ccd_dsens_passes"]
# "<fixture>_<size>_<mode>": a picture derived with the writer (tests/float_tail.py: NAMED), its dense grid 2 / 4 times coarser than the
# picture at non-integer scales on both axes (19 x 50 and 10 x 25 -> 37 x 99) behind a nearest / bicubic final resize
DERIVED = ["rgb192_37x99_nearest", "rgb192_37x99_bicubic"]
SAMPLED = ["rgb192", "cr192", "bicubic190", "bilinear190", "yuv420_8b", "yuv444_10b", "odd100x37"] + DERIVED


def _arch(name):
    """(arch with derived geometry, NN payload, bitdepth, frame_data_type, latent payload, header bytes) of an image fixture, or of
    a derived case by its name."""
    from cool_chic_amd import writer
    from oracle import oracle_py

    if name in DERIVED:
        import float_tail

        oracle_py.build()
        c = float_tail.named(load_golden, oracle_py, name)
        return c.arch, c.triple[1], c.bitdepth, c.frame_data_type, c.triple[2], c.triple[0]
    _, frames = oracle_py.split_stream(load_golden(name)[0])
    (fh, ccs), = frames
    hdr, nn, payload = ccs[0]
    return writer.parse_cc_header(hdr), nn, fh.bitdepth, fh.frame_data_type, payload, hdr


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
    import cool_chic_amd
    from cool_chic_amd import rd

    assert cool_chic_amd.DistortionDeltas.__name__ == "DistortionDeltas"
    assert all(hasattr(cool_chic_amd.DistortionDeltas, m) for m in ("add", "run", "wait", "passes", "delta_map"))
    assert all(hasattr(rd.RdEvaluator, m) for m in ("distortion_delta_map", "cost_delta_map"))


def test_argument_errors_without_a_device():
    from cool_chic_amd._lib import lib

    L = lib()
    arch, nn, _, _, _, _ = _arch("odd18x65")
    h = C.c_void_p()
    assert L.ccd_dsens_create(0, 16, None) == ERR_ARG
    for k in (0, -1, 65, 1 << 20):
        assert L.ccd_dsens_create(0, k, C.byref(h)) == ERR_ARG and not h.value
    handle = C.create_string_buffer(512)  # stands for a handle: the calls must return before they look at it
    d = C.cast(handle, C.c_void_p)
    grid = np.zeros(65 * 18, np.int8)
    lat = (C.c_void_p * arch.n_grids)(*[grid.ctypes.data] * arch.n_grids)
    src = (C.c_void_p * 3)(*[grid.ctypes.data] * 3)
    no_src = (C.c_void_p * 3)(grid.ctypes.data, None, grid.ctypes.data)
    assert L.ccd_dsens_add(None, C.byref(arch), nn, len(nn), lat, src, 8, 0) == ERR_ARG
    assert L.ccd_dsens_add(d, None, nn, len(nn), lat, src, 8, 0) == ERR_ARG
    assert L.ccd_dsens_add(d, C.byref(arch), None, 0, lat, src, 8, 0) == ERR_ARG
    assert L.ccd_dsens_add(d, C.byref(arch), nn, len(nn), None, src, 8, 0) == ERR_ARG
    assert L.ccd_dsens_add(d, C.byref(arch), nn, len(nn), lat, None, 8, 0) == ERR_ARG
    assert L.ccd_dsens_add(d, C.byref(arch), nn, len(nn), lat, no_src, 8, 0) == ERR_ARG
    for bitdepth in (0, 7, 17, -8):
        assert L.ccd_dsens_add(d, C.byref(arch), nn, len(nn), lat, src, bitdepth, 0) == ERR_ARG
    assert L.ccd_dsens_add(d, C.byref(arch), nn, len(nn), lat, src, 8, 3) == ERR_ARG  # a flow "frame" is not scored
    assert bytes(handle) == bytes(512)
    dev = C.c_void_p()
    assert L.ccd_dsens_run(None, None) == ERR_ARG and L.ccd_dsens_wait(None, None) == ERR_ARG
    assert L.ccd_dsens_slot_map(None, 0, 0, C.byref(dev)) == ERR_ARG and not dev.value
    assert L.ccd_dsens_passes(None, 0) == ERR_ARG
    box = (C.c_int32 * 4)()
    assert L.ccd_latent_footprint(None, 0, box) == ERR_ARG and L.ccd_latent_footprint(C.byref(arch), 0, None) == ERR_ARG
    assert L.ccd_latent_footprint(C.byref(arch), -1, box) == ERR_ARG and L.ccd_latent_footprint(C.byref(arch), arch.n_grids, box) == ERR_ARG
    assert L.ccd_latent_probe_stride(C.byref(arch), 0, 3) == ERR_ARG and L.ccd_latent_probe_stride(None, 0, 0) == ERR_ARG


def _shift(arch, g, y, x):
    """Where the box of the latent (y, x) of grid g is anchored, as include/ccd.h states it."""
    lat = [k for k in range(arch.n_grids) if not arch.is_hyperlatent[k]]
    pitch = 1 << lat.index(g)
    return (y * pitch * arch.img_size[0]) // arch.grid_h[lat[0]], (x * pitch * arch.img_size[1]) // arch.grid_w[lat[0]]


def _box_of(arch, g, y, x, box):
    """Rows and columns (inclusive) of the luma box, clipped."""
    sy, sx = _shift(arch, g, y, x)
    H, W = arch.img_size[0], arch.img_size[1]
    return max(sy + box[0], 0), max(sx + box[1], 0), min(sy + box[2], H - 1), min(sx + box[3], W - 1)


@pytest.mark.parametrize("name", ["odd18x65", "rgb192", "bicubic190", "yuv420_8b"] + DERIVED)
def test_footprint_and_strides(name):
    from cool_chic_amd.dsens import latent_footprint, probe_stride

    arch, _, _, fdt, _, _ = _arch(name)
    sh = 1 if fdt == 1 else 0
    prev, n_hyper, strides = None, 0, []
    for g in range(arch.n_grids):
        box = latent_footprint(arch, g)
        S = probe_stride(arch, g, fdt)
        if arch.is_hyperlatent[g]:  # flagged: no footprint, no stride, no passes
            assert box is None and S == 0
            n_hyper += 1
            continue
        top, left, bottom, right = box
        assert top <= 0 <= bottom and left <= 0 <= right
        if prev is not None:  # coarser grids reach at least as far, on every side
            assert top <= prev[0] and left <= prev[1] and bottom >= prev[2] and right >= prev[3], (g, box, prev)
        prev = box
        h, w = arch.grid_h[g], arch.grid_w[g]
        assert 1 <= S <= max(h, w)
        strides.append(S)
        # boxes of neighbours on the lattice are disjoint (chroma boxes too), and S is the smallest stride with that property
        def disjoint(stride):
            for y in range(h - stride):
                a, b = _box_of(arch, g, y, 0, box), _box_of(arch, g, y + stride, 0, box)
                if not (b[0] >> sh) > (a[2] >> sh):
                    return False
            for x in range(w - stride):
                a, b = _box_of(arch, g, 0, x, box), _box_of(arch, g, 0, x + stride, box)
                if not (b[1] >> sh) > (a[3] >> sh):
                    return False
            return True
        assert disjoint(S), (g, S)
        assert S == 1 or not disjoint(S - 1), (g, S)
    assert n_hyper == sum(arch.is_hyperlatent[g] for g in range(arch.n_grids))
    print(name, "strides", strides)
    if name == "odd18x65":  # grids smaller than the stride exist here: their phases are the grid's own positions
        assert any(S >= max(arch.grid_h[g], arch.grid_w[g]) for g, S in zip([g for g in range(arch.n_grids) if not arch.is_hyperlatent[g]], strides))


# ---- GPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cool_chic_amd import DistortionDeltas, _lib

    _lib.lib()
    return DistortionDeltas


FDT_NAMES = ["rgb", "yuv420", "yuv444"]


class _Case:
    """A fixture's architecture and network under random latents, a source decoded from other random latents, one batch of 64
    given-latent slots for the brute force, and the map of a DistortionDeltas handle (16 probe slots) that holds it alone."""

    N = 64

    def __init__(self, name, seed=0):
        import torch

        from cool_chic_amd import DecodeBatch

        self.name = name
        self.arch, self.nn, self.bd, self.fdt, _, _ = _arch(name)
        a = self.arch
        self.n = a.n_grids
        self.hw = [(int(a.grid_h[g]), int(a.grid_w[g])) for g in range(self.n)]
        self.sizes = [h * w for h, w in self.hw]
        self.off = np.concatenate([[0], np.cumsum([(s + 255) // 256 * 256 for s in self.sizes])]).astype(np.int64)
        self.lat = self.random_latents(seed)
        # the brute-force batch: slot k reads row k of one device buffer
        self.buf = torch.zeros((self.N, int(self.off[-1])), dtype=torch.int8, device="cuda")
        self.batch = DecodeBatch(0)
        for k in range(self.N):
            self.batch.add_latents_device(a, self.nn, [self.buf[k].data_ptr() + int(self.off[g]) for g in range(self.n)], self.bd, self.fdt,
                                          owner=self.buf)
        src_planes = self.decode([self.random_latents(seed + 100)])[0]
        self.src = [p.clone() for p in src_planes]
        self.lat_dev = self.device_latents(self.lat)
        self._maps = None

    def random_latents(self, seed):
        rng = np.random.default_rng([seed, len(self.name)])
        lat = [rng.integers(-12, 13, size=hw, dtype=np.int8) for hw in self.hw]
        for a in lat:  # the alphabet's ends: a corner each, and a few positions anywhere
            a.flat[0], a.flat[-1] = -64, 63
            where = rng.choice(a.size, size=min(a.size, 6), replace=False)
            a.flat[where] = rng.choice([-64, 63], size=len(where))
        return lat

    def flat(self, lat):
        row = np.zeros(int(self.off[-1]), np.int8)
        for g, a in enumerate(lat):
            row[self.off[g]:self.off[g] + a.size] = a.ravel()
        return row

    def device_latents(self, lat):
        import torch

        return torch.from_numpy(self.flat(lat)).cuda()

    def ptrs(self, dev_row):
        return [dev_row.data_ptr() + int(self.off[g]) for g in range(self.n)]

    def decode(self, lats):
        """Planes (CUDA tensors, valid until the next call) of up to 64 latent sets through the given-latent slots."""
        import torch

        assert len(lats) <= self.N
        host = np.stack([self.flat(l) for l in lats] + [self.flat(lats[0])] * (self.N - len(lats)))
        self.buf.copy_(torch.from_numpy(host))
        torch.cuda.synchronize()
        self.batch.run(); self.batch.wait()
        return [[torch.as_tensor(self.batch.plane_device(k, p), device="cuda") for p in range(3)] for k in range(len(lats))]

    def sse(self, lats):
        from cool_chic_amd.quality import QualityMeter

        out = []
        with QualityMeter(0) as meter:
            for i in range(0, len(lats), self.N):
                planes = self.decode(lats[i:i + self.N])
                q = meter.score_planes(planes, [self.src] * len(planes), [self.bd] * len(planes), [FDT_NAMES[self.fdt]] * len(planes), ms_ssim=False)
                out += [sum(int(v) for v in r.sse) for r in q]
        return out

    def brute(self, moves, lat=None):
        """[(g, y, x, s)] -> the reference entries: SSE(moved) - SSE(base), or SENTINEL where the move leaves the alphabet."""
        lat = self.lat if lat is None else lat
        cands, legal = [lat], []
        for g, y, x, s in moves:
            ok = -64 <= int(lat[g][y, x]) + s <= 63
            legal.append(ok)
            if ok:
                l2 = list(lat)
                l2[g] = lat[g].copy()
                l2[g][y, x] += s
                cands.append(l2)
        sse = self.sse(cands)
        it = iter(sse[1:])
        return [next(it) - sse[0] if ok else SENTINEL for ok in legal]

    def run_maps(self, handle, slot):
        import torch

        return [torch.as_tensor(handle.delta_map(slot, g), device="cuda").cpu().numpy() for g in range(self.n)]

    def maps(self, gpu):
        if self._maps is None:
            d = gpu(0, 16)
            d.add(self.arch, self.nn, self.ptrs(self.lat_dev), [t.data_ptr() for t in self.src], self.bd, self.fdt, owner=(self.lat_dev, self.src))
            d.run(); d.wait()
            self._maps = self.run_maps(d, 0)
            self.n_passes = d.passes(0)
            d.close()
            for g, m in enumerate(self._maps):
                assert m.shape == (2,) + self.hw[g] and m.dtype == np.int64
        return self._maps


_CASES = {}


def _case(name):
    if name not in _CASES:
        _CASES[name] = _Case(name)
    return _CASES[name]


def _compare(case, maps, moves, want):
    bad = [(mv, int(maps[mv[0]][(mv[3] + 1) // 2, mv[1], mv[2]]), w) for mv, w in zip(moves, want)
           if int(maps[mv[0]][(mv[3] + 1) // 2, mv[1], mv[2]]) != w]
    assert not bad, (case.name, len(bad), len(moves), bad[:6])


@pytest.mark.gpu
def test_every_latent_of_a_tiny_picture(gpu):
    """18 x 65: grids down to 1 x 3 and 1 x 2 (smaller than any stride), boxes clipped on every side, hyperlatent grids."""
    case = _case("odd18x65")
    maps = case.maps(gpu)
    moves = [(g, y, x, s) for g in range(case.n) for y in range(case.hw[g][0]) for x in range(case.hw[g][1]) for s in (-1, 1)]
    want = case.brute(moves)
    assert len(moves) == 2 * sum(case.sizes) and sum(w != SENTINEL for w in want) > 2500
    _compare(case, maps, moves, want)
    real = [w for mv, w in zip(moves, want) if w != SENTINEL and not case.arch.is_hyperlatent[mv[0]]]
    assert min(real) < 0 < max(real)  # the deltas take both signs
    for g in range(case.n):
        if case.arch.is_hyperlatent[g]:  # does not feed the synthesis: zeros, and the sentinel at the alphabet's ends
            m = maps[g]
            assert np.array_equal(m[0] == SENTINEL, case.lat[g] == -64) and np.array_equal(m[1] == SENTINEL, case.lat[g] == 63)
            assert not m[m != SENTINEL].any()
    print(f"odd18x65: {len(moves)} entries, {case.n_passes} passes, dD in [{min(real)}, {max(real)}]")


def _sample_positions(h, w, rng):
    pos = {(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2), (h // 2, 0), (h // 2, w - 1)}
    want = min(h * w, len(pos) + 24)
    while len(pos) < want:
        pos.add((int(rng.integers(h)), int(rng.integers(w))))
    return sorted(pos)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SAMPLED)
def test_sampled_latents(gpu, name):
    case = _case(name)
    maps = case.maps(gpu)
    rng = np.random.default_rng(7)
    moves = [(g, y, x, s) for g in range(case.n) for y, x in _sample_positions(*case.hw[g], rng) for s in (-1, 1)]
    want = case.brute(moves)
    _compare(case, maps, moves, want)
    real = [w for w in want if w != SENTINEL]
    assert SENTINEL in want and min(real) < 0 < max(real)
    # and the sentinels of the whole map sit exactly at the alphabet's ends
    for g in range(case.n):
        assert np.array_equal(maps[g][0] == SENTINEL, case.lat[g] == -64) and np.array_equal(maps[g][1] == SENTINEL, case.lat[g] == 63)
    print(f"{name}: {len(moves)} entries equal, {case.n_passes} passes, dD in [{min(real)}, {max(real)}]")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rgb192", "bicubic190"] + DERIVED)
def test_footprint_by_impulse(gpu, name):
    """Three networks (the perturbation recipe of test_given_latents.py: weights only), single latents flipped between the
    alphabet's ends at the corners and the centre of every grid: no sample outside ccd_latent_footprint's box changes."""
    import torch
    from test_given_latents import _perturbed_networks

    from cool_chic_amd import DecodeBatch
    from cool_chic_amd.dsens import latent_footprint
    from oracle import oracle_py

    case = _case(name)
    arch0, nn0, bd, fdt, payload, hdr = _arch(name)
    nn_ints = oracle_py.decode_coolchic(hdr, nn0, payload, stop_after_entropy=True)["nn_ints"]
    nets = _perturbed_networks(arch0, nn_ints)
    assert len(nets) == 3
    sh = 1 if fdt == 1 else 0
    n_changed = 0
    for arch, nn in nets:
        b = DecodeBatch(0)
        flips = []
        b.add_latents(arch, nn, case.lat, bd, fdt)
        for g in range(case.n):
            if arch.is_hyperlatent[g]:
                continue
            h, w = case.hw[g]
            for y, x in sorted({(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2)}):
                l2 = list(case.lat)
                l2[g] = case.lat[g].copy()
                l2[g][y, x] = 63 if l2[g][y, x] < 0 else -64
                b.add_latents(arch, nn, l2, bd, fdt)
                flips.append((g, y, x))
        b.run(); b.wait()
        base = b.planes(0)
        for k, (g, y, x) in enumerate(flips):
            y0, x0, y1, x1 = _box_of(arch, g, y, x, latent_footprint(arch, g))
            for p, (got, ref) in enumerate(zip(b.planes(k + 1), base)):
                s = sh if p else 0
                diff = got != ref
                n_changed += int(diff.sum())
                diff[y0 >> s:(y1 >> s) + 1, x0 >> s:(x1 >> s) + 1] = False
                assert not diff.any(), (name, g, y, x, p, np.argwhere(diff)[:4].tolist(), (y0, x0, y1, x1))
        b.close()
    assert n_changed > 1000  # the flips did move samples
    torch.cuda.synchronize()


def _equal_maps(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
def test_independence(gpu):
    """The map does not depend on the number of probe slots, on what else the handle holds, or on the run; the caller's latents are
    read only (sentinel bytes around every grid, as test_given_latents._device_buffer lays them out)."""
    from test_given_latents import _device_buffer

    cases = [_case(n) for n in ("odd18x65", "rgb192", "yuv420_8b")]
    want = [c.maps(gpu) for c in cases]
    for k in (1, 5):
        for c, w in zip(cases[:2], want[:2]):
            d = gpu(0, k)
            d.add(c.arch, c.nn, c.ptrs(c.lat_dev), [t.data_ptr() for t in c.src], c.bd, c.fdt)
            d.run(); d.wait()
            assert d.passes(0) == c.n_passes
            assert _equal_maps(c.run_maps(d, 0), w), (c.name, k)
            d.close()
    d = gpu(0, 16)
    bufs = []
    for c in cases:
        buf, pos = _device_buffer(c.lat, offsets=[1, 3, 7])
        d.add(c.arch, c.nn, [buf.data_ptr() + p for p in pos], [t.data_ptr() for t in c.src], c.bd, c.fdt, owner=buf)
        bufs.append((buf, buf.cpu().numpy().copy()))
    for run in range(2):
        d.run(); d.wait()
        for s, (c, w) in enumerate(zip(cases, want)):
            assert _equal_maps(c.run_maps(d, s), w), (c.name, "run", run)
    for buf, before in bufs:
        assert np.array_equal(buf.cpu().numpy(), before)
    d.close()


@pytest.mark.gpu
def test_latents_changed_in_place_and_alphabet(gpu):
    import torch

    from cool_chic_amd._lib import CcdError

    case = _case("odd100x37")
    want_a = case.maps(gpu)
    lat_b = case.random_latents(5)
    dev = case.lat_dev.clone()
    d = gpu(0, 16)
    d.add(case.arch, case.nn, case.ptrs(dev), [t.data_ptr() for t in case.src], case.bd, case.fdt, owner=dev)
    d.run(); d.wait()
    assert _equal_maps(case.run_maps(d, 0), want_a)
    dev.copy_(torch.from_numpy(case.flat(lat_b)))
    torch.cuda.synchronize()
    d.run(); d.wait()
    maps_b = case.run_maps(d, 0)
    assert not _equal_maps(maps_b, want_a)
    rng = np.random.default_rng(11)
    moves = [(g, y, x, s) for g in range(case.n) for y, x in _sample_positions(*case.hw[g], rng)[:6] for s in (-1, 1)]
    _compare(case, maps_b, moves, case.brute(moves, lat_b))
    # a base latent outside the alphabet: that slot's CCD_ERR_VALUE at wait, the slot beside it untouched; fine again once repaired
    good = case.device_latents(lat_b)
    d.add(case.arch, case.nn, case.ptrs(good), [t.data_ptr() for t in case.src], case.bd, case.fdt, owner=good)
    bad = case.flat(lat_b)
    bad[int(case.off[2]) + 3] = 64
    dev.copy_(torch.from_numpy(bad))
    torch.cuda.synchronize()
    d.run()
    with pytest.raises(CcdError) as e:
        d.wait()
    assert e.value.code == ERR_VALUE
    with pytest.raises(CcdError) as e:
        d.delta_map(0, 0)
    assert e.value.code == ERR_VALUE
    assert _equal_maps(case.run_maps(d, 1), maps_b)
    dev.copy_(torch.from_numpy(case.flat(lat_b)))
    torch.cuda.synchronize()
    d.run(); d.wait()
    assert _equal_maps(case.run_maps(d, 0), maps_b) and _equal_maps(case.run_maps(d, 1), maps_b)
    d.close()


@pytest.mark.gpu
def test_rd_evaluator(gpu, oracle):
    """evaluate(distortion_deltas=True) returns what evaluate() returns, and cost_delta_map is the cost of the moved candidate minus
    the base's, both from plain evaluate calls.  The distortion term is formed from the same exact integers on both sides; the
    rate term may differ by test_rate_deltas.py's bound (2 (1 + |dep|) TERM_TOL + |ref| 2^-23 bits), scaled by lmbda / n_pixels."""
    import torch
    from test_rate_deltas import _Case as RateCase

    from cool_chic_amd import RdEvaluator
    from cool_chic_amd.quality import _planes_to_frame_data

    case = _case("rgb192")
    _, _, _, _, payload, hdr = _arch("rgb192")
    geo = RateCase(oracle, "rgb192", hdr, case.nn, payload, planes=False)  # the dependents of a latent: geometry only
    source = _planes_to_frame_data([t.cpu().numpy() for t in case.src], case.bd, FDT_NAMES[case.fdt])
    lmbda = 1e-3
    rng = np.random.default_rng(3)
    moves = []
    while len(moves) < 10:
        g = int(rng.integers(case.n))
        y, x, s = int(rng.integers(case.hw[g][0])), int(rng.integers(case.hw[g][1])), int(rng.choice([-1, 1]))
        if -64 <= int(case.lat[g][y, x]) + s <= 63:
            moves.append((g, y, x, s))
    ev = RdEvaluator(0)
    ev.add(case.arch, case.nn, case.lat, source)
    plain = ev.evaluate(lmbda)
    both = ev.evaluate(lmbda, rate_deltas=True, distortion_deltas=True)
    assert len(plain) == len(both) == 1
    for a, b in zip(plain, both):
        assert a.rate.status == b.rate.status == 0 and a.rate.bits.tolist() == b.rate.bits.tolist()
        assert a.quality.sse == b.quality.sse and (a.mse, a.bits, a.cost) == (b.mse, b.bits, b.cost)
    dd = [torch.as_tensor(ev.distortion_delta_map(0, g), device="cuda").cpu().numpy() for g in range(case.n)]
    assert _equal_maps(dd, case.maps(gpu))
    cost_maps = [ev.cost_delta_map(0, g, lmbda) for g in range(case.n)]
    for g, m in enumerate(cost_maps):
        assert m.dtype == torch.float64 and tuple(m.shape) == (2,) + case.hw[g] and m.is_cuda
        m = m.cpu().numpy()
        assert np.array_equal(np.isposinf(m), dd[g] == SENTINEL) and np.isfinite(m[dd[g] != SENTINEL]).all()
    ev2 = RdEvaluator(0)
    ev2.add(case.arch, case.nn, case.lat, source)
    for g, y, x, s in moves:
        l2 = list(case.lat)
        l2[g] = case.lat[g].copy()
        l2[g][y, x] += s
        ev2.add(case.arch, case.nn, l2, source)
    cands = ev2.evaluate(lmbda)
    base = cands[0]
    assert (base.mse, base.bits, base.cost) == (plain[0].mse, plain[0].bits, plain[0].cost)
    n_pixels, n_samples, maxv = source.n_pixels, sum(base.quality.n), float(2 ** case.bd - 1)
    for (g, y, x, s), c in zip(moves, cands[1:]):
        d_sse = sum(c.quality.sse) - sum(base.quality.sse)
        assert d_sse == int(dd[g][(s + 1) // 2, y, x])  # the distortion side contributes exactly
        d_bits = c.bits - base.bits
        ref = float(d_sse) / (float(n_samples) * maxv * maxv) + lmbda * d_bits / float(n_pixels)
        got = float(cost_maps[g][(s + 1) // 2, y, x])
        bound = lmbda / float(n_pixels) * geo.bound(g, y, x, d_bits)
        print(f"rgb192 grid {g} ({y}, {x}) {s:+d}: map {got!r} evaluate {ref!r} |diff| {abs(got - ref):.3g} bound {bound:.3g}; "
              f"cost(moved) - cost(base) {c.cost - base.cost!r}")
        assert abs(got - ref) <= bound, (g, y, x, s, got, ref, bound)
    ev.close(); ev2.close()
