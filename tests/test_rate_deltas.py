"""Rate sensitivity (ccd_enc_measure_deltas, EncodeBatch.measure_deltas / delta_map, DESIGN.md section 4.10 "Rate sensitivity"):
for every latent the exact change of the slot's model bits if that one latent were v - 1 or v + 1.

The reference is the CPU oracle, never the code under test.  For a position p and a sign the latents with that one value
changed go through the host writer (writer.encode_coolchic), the oracle entropy-decodes the bytes
(oracle.decode_coolchic(stop_after_entropy=True): latents and (mu, scale) table indices in decode order),
oracle.laplace_bounds gives every interval and numpy float64 every pixel's 24 - log2(width): test_device_rate._reference,
restated here with one cache of laplace_bounds for all the decodes.  The reference value is total_bits(perturbed) -
total_bits(base), formed as ONE math.fsum over the pixels whose bits differ (+ the perturbed, - the base ones): the correctly
rounded difference of the two exact sums - subtracting two separately rounded totals of ~3e4 bits would lose 4e-12, more
than the bound below allows a latent with few dependents.

Bound: |dev - ref| <= 2 (1 + |dep(p)|) TERM_TOL + |ref| 2^-23.  TERM_TOL = 24 * 2^-48 is the project's bound per log2 term
(test_device_rate.py), there are 2 (1 + |dep|) such terms, |ref| 2^-23 covers the one float32 rounding of the stored value.
|dep(p)| is computed here from the context template (arm.py:501-509) and the grids' geometry, not taken from the library."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import ROOT, load_golden

ERR_VALUE, ERR_ARG = -2, -7
ENTRY_POINTS = ["ccd_enc_measure_deltas", "ccd_enc_slot_delta_map"]
TERM_TOL = 24.0 * 2.0 ** -48
FIXTURES = ["odd18x65", "odd100x37", "vid3_ldp"]
# arm.py:501-509: priority of each of the 40 causal positions of the 9 x 9 mask, row-major; the k-th context is the position of rank k
PRIORITY = [38, 35, 30, 25, 23, 31, 36, 37, 39, 33, 28, 21, 20, 6, 15, 22, 29, 34, 32, 18,
            12, 10, 5, 9, 14, 19, 27, 24, 13, 8, 2, 1, 3, 11, 17, 26, 16, 7, 4, 0]


# ---- CPU -------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_exported():
    from cool_chic_amd import _lib

    with open(os.path.join(ROOT, "include", "ccd.h")) as f:
        header = f.read()
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert name + "(" in header, name
        assert name in _lib.SIGNATURES, name
        assert getattr(L, name) is not None
    from cool_chic_amd import rd
    from cool_chic_amd.encoder import EncodeBatch

    assert all(hasattr(EncodeBatch, m) for m in ("measure_deltas", "delta_map"))
    assert hasattr(rd.RdEvaluator, "rate_delta_map")


def test_null_arguments_are_argument_errors_without_a_device():
    from cool_chic_amd._lib import lib

    L = lib()
    dev = C.c_void_p()
    assert L.ccd_enc_measure_deltas(None, None) == ERR_ARG
    assert L.ccd_enc_slot_delta_map(None, 0, 0, C.byref(dev)) == ERR_ARG and not dev.value
    assert L.ccd_enc_slot_delta_map(None, 0, 0, None) == ERR_ARG


# ---- the reference ---------------------------------------------------------------------------------------------------
def _cool_chics(oracle, bs):
    _, frames = oracle.split_stream(bs)
    return [cc for _, ccs in frames for cc in ccs]


_WIDTH = {}  # (mu index << 24 | scale index << 8 | symbol + 64) -> right - left of oracle.laplace_bounds


def _bit_planes(oracle, hdr, nn, lat):
    """([int8 (h, w)] latents, [float64 (h, w)] 24 - log2(width) of every latent, raster): test_device_rate._reference."""
    r = oracle.decode_coolchic(hdr, nn, lat, stop_after_entropy=True)
    planes = []
    for g in range(r["n_grids"]):
        h, w = r["grid_hw"][g]
        yy, xx = np.mgrid[0:h, 0:w]
        y, x = yy.ravel(), xx.ravel()
        order = np.arange(h * w) if w <= 9 else np.lexsort((y, x + 10 * y))  # raster index of the k-th decoded pixel
        ms = r["mu_scale_idx"][g].astype(np.int64)
        sym = r["latent"][g].ravel()[order].astype(np.int64)
        triple = (ms[:, 0] << 24) | (ms[:, 1] << 8) | (sym + 64)
        uniq, inv = np.unique(triple, return_inverse=True)
        wu = np.empty(len(uniq), np.int64)
        for k, t in enumerate(uniq.tolist()):
            if t not in _WIDTH:
                left, right = oracle.laplace_bounds(t >> 24, (t >> 8) & 0xFFFF, (t & 0xFF) - 64)
                _WIDTH[t] = right - left
            wu[k] = _WIDTH[t]
        width = np.empty(h * w, np.int64)
        width[order] = wu[inv]
        assert width.min(initial=1) >= 1 and width.max(initial=1) <= 1 << 24
        planes.append(24.0 - np.log2(width.astype(np.float64)).reshape(h, w))
    return [np.ascontiguousarray(a) for a in r["latent"]], planes


class _Case:
    """One cool-chic: architecture, NN payload, latents, the base bit planes and the geometry dep(p) follows from."""

    def __init__(self, oracle, name, hdr, nn, lat, latents=None, planes=True):
        from cool_chic_amd import writer

        self.name, self.oracle, self.nn = name, oracle, nn
        self.arch = writer.parse_cc_header(hdr)
        if latents is not None:  # other latents under the same networks: their bytes come from the host writer
            hdr, nn, lat = self._write(latents)
        if planes:
            self.latents, self.base = _bit_planes(oracle, hdr, nn, lat)
        else:  # geometry and latents only
            self.latents = [np.ascontiguousarray(a) for a in oracle.decode_coolchic(hdr, nn, lat, stop_after_entropy=True)["latent"]]
        a = self.arch
        self.n = a.n_grids
        self.hw = [(int(a.grid_h[g]), int(a.grid_w[g])) for g in range(self.n)]
        self.level = [0] * self.n  # size changes between grid 0 and grid g
        for g in range(1, self.n):
            self.level[g] = self.level[g - 1] + (self.hw[g] != self.hw[g - 1])
        self.ifce_in = [int(a.input_features_ifce[g]) for g in range(self.n)]
        self.n_sp = int(a.spatial_context_arm)
        self.taps = [None] * self.n_sp  # (dy, dx): context k of (y, x) is the latent at (y - dy, x + dx)
        for pos, rank in enumerate(PRIORITY):
            if rank < self.n_sp:
                self.taps[rank] = (4 - pos // 9, pos % 9 - 4)
        self.n_decodes = 0

    def _write(self, latents):
        from cool_chic_amd import writer

        cc = writer.encode_coolchic(self.arch, self.nn, latents)
        h2 = writer.parse_cc_header(cc)
        p, q = h2.n_bytes_header, h2.n_bytes_header + h2.nn_n_bytes
        assert cc[p:q] == self.nn
        return cc[:p], cc[p:q], cc[q:]

    def spatial_dependents(self, m, y, x):
        h, w = self.hw[m]
        out = [(y + dy, x - dx) for dy, dx in self.taps]
        return [(qy, qx) for qy, qx in out if 0 <= qy < h and 0 <= qx < w]

    def ifce_blocks(self, m, y, x):
        """[(fine grid g, rows, columns)]: the pixels of g whose feature reads (m, y, x), ((qy >> 1) >> sh, (qx >> 1) >> sh) == (y, x)."""
        out = []
        for g in range(m):
            if self.ifce_in[g] > 0 and g != self.n - 1 and m - g - 1 < self.ifce_in[g]:
                side = 2 << (self.level[m] - self.level[g + 1])
                h, w = self.hw[g]
                rows, cols = range(y * side, min((y + 1) * side, h)), range(x * side, min((x + 1) * side, w))
                if len(rows) and len(cols):
                    out.append((g, rows, cols))
        return out

    def n_dep(self, m, y, x):
        return len(self.spatial_dependents(m, y, x)) + sum(len(r) * len(c) for _, r, c in self.ifce_blocks(m, y, x))

    def bound(self, m, y, x, ref):
        return 2.0 * (1 + self.n_dep(m, y, x)) * TERM_TOL + abs(ref) * 2.0 ** -23

    def reference(self, m, y, x, sign):
        """total_bits(latents with (m, y, x) moved by sign) - total_bits(latents), one fsum over the pixels that differ."""
        lat = [a.copy() for a in self.latents]
        lat[m][y, x] += sign
        got, planes = _bit_planes(self.oracle, *self._write(lat))
        assert all(np.array_equal(a, b) for a, b in zip(got, lat))
        self.n_decodes += 1
        terms, moved = [], set()
        for g, (new, old) in enumerate(zip(planes, self.base)):
            idx = new != old
            terms += new[idx].tolist() + (-old[idx]).tolist()
            moved |= {(g, int(qy), int(qx)) for qy, qx in zip(*np.nonzero(idx))}
        # every pixel whose bits moved is p or one of dep(p) as THIS file derives it
        allowed = {(m, y, x)} | {(m, qy, qx) for qy, qx in self.spatial_dependents(m, y, x)}
        for g, rows, cols in self.ifce_blocks(m, y, x):
            allowed |= {(g, qy, qx) for qy in rows for qx in cols}
        assert moved <= allowed, (self.name, m, y, x, sorted(moved - allowed)[:4])
        return math.fsum(terms)


def _positions(case, m, rng):
    """[(y, x, signs)] of grid m: everything (both signs) up to 64 symbols, else 48 seeded positions with the four corners, one
    position on each edge and one whose spatial dependents the right border cuts (these nine with both signs), the other 39
    with one seeded sign each."""
    h, w = case.hw[m]
    lat = case.latents[m]
    legal = lambda y, x, s: -64 <= int(lat[y, x]) + s <= 63  # noqa: E731
    if h * w <= 64:
        return [(y, x, [s for s in (-1, 1) if legal(y, x, s)]) for y in range(h) for x in range(w)]
    must = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 3), (h // 2, 0), (h // 3, w - 1)]
    cut = (h // 2, w - 1)  # a later pixel of its row / the rows below would hold it in a tap, were the grid wider
    assert len(case.spatial_dependents(m, *cut)) < len(case.spatial_dependents(m, h // 2, w // 2))
    must.append(cut)
    must = list(dict.fromkeys(must))
    rest = [(y, x) for y in range(h) for x in range(w) if (y, x) not in set(must)]
    picks = must + [rest[i] for i in rng.choice(len(rest), size=48 - len(must), replace=False)]
    out = []
    for k, (y, x) in enumerate(picks):
        if k < len(must):
            out.append((y, x, [s for s in (-1, 1) if legal(y, x, s)]))
            continue
        s = -1 if (k + int(rng.integers(2))) % 2 else 1
        out.append((y, x, [s if legal(y, x, s) else -s]))
    return out


# ---- GPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cool_chic_amd import EncodeBatch, _lib

    _lib.lib()
    return EncodeBatch


def _maps(enc, slot, n_grids):
    import torch

    return [torch.as_tensor(enc.delta_map(slot, g), device="cuda").cpu().numpy() for g in range(n_grids)]


def _words(maps):
    return [m.view(np.uint32).tolist() for m in maps]


def _bits64(rate):
    return np.concatenate([rate.bits, [rate.total_bits]]).astype(np.float64).view(np.uint64).tolist()


def _check(case, maps, checks, what):
    """Every (m, y, x, sign, ref) against the map; returns the largest |dev - ref| / bound."""
    worst = 0.0
    for m, y, x, sign, ref in checks:
        dev = float(maps[m][(sign + 1) // 2, y, x])
        bound = case.bound(m, y, x, ref)
        err = abs(dev - ref)
        worst = max(worst, err / bound)
        assert err <= bound, (what, case.name, m, y, x, sign, dev, ref, err, bound)
    return worst


@pytest.fixture(scope="module")
def cases(oracle):
    """The three cool-chics and their references, computed once: {name: (case, [(grid, y, x, sign, reference)])}."""
    out = {}
    for name in FIXTURES:
        hdr, nn, lat = _cool_chics(oracle, load_golden(name)[0])[0]
        case = _Case(oracle, name, hdr, nn, lat)
        rng = np.random.default_rng(1234)
        checks = []
        for m in range(case.n):
            for y, x, signs in _positions(case, m, rng):
                checks += [(m, y, x, s, case.reference(m, y, x, s)) for s in signs]
        # the cap on the oracle's work: 2 x 64 for every small grid at the most, 9 x 2 + 39 = 57 for a large one; vid3_ldp (four
        # small grids of 8, 8, 28, 28 symbols, six large ones) is the largest with 144 + 342 = 486
        assert case.n_decodes <= 500, (name, case.n_decodes)
        out[name] = (case, checks)
    return out


@pytest.fixture(scope="module")
def measured(gpu, cases):
    """The three in one handle, one measure_deltas: (handle, {name: maps})."""
    enc = gpu(0)
    for name in FIXTURES:
        case = cases[name][0]
        enc.add(case.arch, case.nn, case.latents)
    enc.measure_deltas()
    enc.wait()
    maps = {name: _maps(enc, s, cases[name][0].n) for s, name in enumerate(FIXTURES)}
    yield enc, maps
    enc.close()


def test_the_fixtures_reach_every_kind_of_dependent(oracle):
    """Geometry only: a grid with two or more IFCE sources, a dependent block of side >= 4, W <= 9 raster grids down to 1 x 2."""
    geo = {name: _Case(oracle, name, *_cool_chics(oracle, load_golden(name)[0])[0], planes=False) for name in FIXTURES}
    assert any(f >= 2 for case in geo.values() for f in case.ifce_in)
    sides = [len(r) for case in geo.values() for m in range(case.n) for _, r, _ in case.ifce_blocks(m, 0, 0)]
    assert max(sides) >= 4
    assert (1, 2) in geo["odd100x37"].hw and (2, 1) in geo["odd18x65"].hw
    assert any(w <= 9 for _, w in geo["odd18x65"].hw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_parity_with_the_oracle(cases, measured, name):
    case, checks = cases[name]
    maps = measured[1][name]
    for g, mp in enumerate(maps):
        assert mp.dtype == np.float32 and mp.shape == (2,) + case.hw[g]
        assert np.array_equal(np.isinf(mp[0]), case.latents[g] == -64) and np.array_equal(np.isinf(mp[1]), case.latents[g] == 63)
        assert not np.isnan(mp).any()
    worst = _check(case, maps, checks, "parity")
    n_big = max(case.n_dep(m, y, x) for m, y, x, _, _ in checks)
    print(f"{name}: {len(checks)} (position, sign) pairs, {case.n_decodes} oracle decodes, up to {n_big} dependents, "
          f"worst deviation {worst:.3g} of the bound")


@pytest.mark.gpu
def test_alphabet_edges(gpu, oracle, cases):
    base = cases["odd18x65"][0]
    lat = [a.copy() for a in base.latents]
    hi, lo, coarse = (0, 30, 7), (0, 41, 11), (3, 4, 1)
    lat[hi[0]][hi[1:]] = 63
    lat[lo[0]][lo[1:]] = -64
    lat[coarse[0]][coarse[1:]] = 63
    hdr, nn, payload = _cool_chics(oracle, load_golden("odd18x65")[0])[0]
    case = _Case(oracle, "odd18x65 with 63 / -64", hdr, nn, payload, latents=lat)
    assert all(np.array_equal(a, b) for a, b in zip(case.latents, lat))
    enc = gpu(0)
    enc.add(case.arch, case.nn, lat)
    enc.measure_deltas()
    enc.wait()
    maps = _maps(enc, 0, case.n)
    enc.close()
    for g, mp in enumerate(maps):  # +inf exactly where the move leaves the alphabet
        assert np.array_equal(np.isinf(mp[0]), lat[g] == -64) and np.array_equal(np.isinf(mp[1]), lat[g] == 63), g
        assert not np.isnan(mp).any() and not (mp == -np.inf).any()
    assert maps[0][1, 30, 7] == np.inf and maps[0][0, 41, 11] == np.inf and maps[3][1, 4, 1] == np.inf
    checks = []
    for (m, y, x), sign in ((hi, -1), (lo, 1), (coarse, -1)):
        checks.append((m, y, x, sign, case.reference(m, y, x, sign)))  # the opposite plane there
        for ny, nx in ((y, x - 1), (y - 1, x), (y, x + 1)):            # neighbours: the edge value is a context of theirs or they of it
            for s in (-1, 1):
                if -64 <= int(lat[m][ny, nx]) + s <= 63:
                    checks.append((m, ny, nx, s, case.reference(m, ny, nx, s)))
    worst = _check(case, maps, checks, "edges")
    print(f"alphabet edges: {len(checks)} pairs, worst deviation {worst:.3g} of the bound")


@pytest.mark.gpu
def test_the_base_results_are_the_meters(gpu, cases, measured):
    enc, _ = measured
    other = gpu(0)
    for name in FIXTURES:
        case = cases[name][0]
        other.add(case.arch, case.nn, case.latents)
    other.measure()
    other.wait()
    for s in range(len(FIXTURES)):
        a, b = enc.rate(s), other.rate(s)
        assert a.status == b.status == 0 and _bits64(a) == _bits64(b), s
        assert a.sum_width.tolist() == b.sum_width.tolist() and a.n_symbols.tolist() == b.n_symbols.tolist()
        assert (a.n_bytes_nn, a.n_bytes_header) == (b.n_bytes_nn, b.n_bytes_header)
    other.close()


@pytest.mark.gpu
def test_a_slot_gives_the_same_maps_alone_in_a_batch_and_twice(gpu, oracle, cases, measured):
    from cool_chic_amd import writer

    case = cases["odd100x37"][0]
    want = _words(measured[1]["odd100x37"])  # slot 1 of three
    alone = gpu(0)
    alone.add(case.arch, case.nn, case.latents)
    alone.measure_deltas(); alone.wait()
    assert _words(_maps(alone, 0, case.n)) == want
    alone.measure_deltas(); alone.wait()  # a second call
    assert _words(_maps(alone, 0, case.n)) == want
    alone.close()
    # behind two slots of other architectures (rgb192: another ARM; kodim14: 20 contexts, other grids)
    mixed = gpu(0)
    for name in ("kodim14", "rgb192"):
        hdr, nn, lat = _cool_chics(oracle, load_golden(name)[0])[0]
        mixed.add(writer.parse_cc_header(hdr), nn, oracle.decode_coolchic(hdr, nn, lat, stop_after_entropy=True)["latent"])
    assert mixed.add(case.arch, case.nn, case.latents) == 2
    mixed.measure_deltas(); mixed.wait()
    assert _words(_maps(mixed, 2, case.n)) == want
    mixed.close()


def _decoded(names, oracle, bitdepth=0):
    from cool_chic_amd import DecodeBatch

    dec = DecodeBatch(0)
    for name in names:
        hdr, nn, lat = _cool_chics(oracle, load_golden(name)[0])[0]
        dec.add(hdr, nn, lat, bitdepth, 0)
    dec.run(); dec.wait()
    return dec


def _device_grid(dec, slot, g):
    import torch

    from cool_chic_amd._lib import lib
    from cool_chic_amd.batch import _DevArray

    h = dec.header(slot)
    return torch.as_tensor(_DevArray(lib().ccd_batch_latent(dec._h, slot, g), (h.grid_h[g], h.grid_w[g]), "|i1", dec), device="cuda")


@pytest.mark.gpu
def test_device_latents_are_read_at_the_call(gpu, oracle, cases):
    import torch

    case = cases["odd100x37"][0]
    dec = _decoded(["odd100x37"], oracle)
    enc = gpu(0)
    enc.add_from_decode(dec, 0)
    enc.measure_deltas(); enc.wait()
    first = _maps(enc, 0, case.n)
    m, y, x = 1, 9, 20
    plane = _device_grid(dec, 0, m)
    v = int(case.latents[m][y, x])
    new = v + 1 if v < 63 else v - 1
    plane[y, x] = new
    torch.cuda.synchronize()
    enc.measure_deltas(); enc.wait()
    second = _maps(enc, 0, case.n)
    lat = [a.copy() for a in case.latents]
    lat[m][y, x] = new
    fresh = gpu(0)
    fresh.add(case.arch, case.nn, lat)
    fresh.measure_deltas(); fresh.wait()
    assert _words(second) == _words(_maps(fresh, 0, case.n))
    fresh.close()
    # the maps moved where the changed latent is read: at its dependents (their own term is priced under another model)
    dep = [(m, qy, qx) for qy, qx in case.spatial_dependents(m, y, x)]
    for g, rows, cols in case.ifce_blocks(m, y, x):
        dep += [(g, qy, qx) for qy in rows for qx in cols]
    changed = [not np.array_equal(first[g][:, qy, qx], second[g][:, qy, qx]) for g, qy, qx in dep]
    assert len(dep) > case.n_sp and sum(changed) > len(dep) // 2, (sum(changed), len(dep))
    enc.close(); dec.close()


@pytest.mark.gpu
def test_poisoned_device_latent_is_that_slots_error_only(gpu, oracle, cases):
    import torch

    from cool_chic_amd._lib import CcdError

    names = ["odd18x65", "rgb192", "odd100x37"]
    dec = _decoded(names, oracle)
    plane = _device_grid(dec, 1, 2)
    keep = plane.clone()
    plane.fill_(64)
    torch.cuda.synchronize()
    enc = gpu(0)
    for s in range(3):
        enc.add_from_decode(dec, s)
    enc.measure_deltas()
    with pytest.raises(CcdError) as e:
        enc.wait()
    assert e.value.code == ERR_VALUE
    assert enc.rate(1).status == ERR_VALUE
    with pytest.raises(CcdError) as e:
        enc.delta_map(1, 0)
    assert e.value.code == ERR_VALUE
    for s in (0, 2):
        case, checks = cases[names[s]]
        assert enc.rate(s).status == 0
        _check(case, _maps(enc, s, case.n), checks, "beside a poisoned slot")
    plane.copy_(keep)  # clean again: the next call succeeds for every slot
    torch.cuda.synchronize()
    enc.measure_deltas(); enc.wait()
    assert all(enc.rate(s).status == 0 for s in range(3))
    assert all(np.isfinite(m).any() for m in _maps(enc, 1, dec.header(1).n_grids))
    case, checks = cases[names[0]]
    _check(case, _maps(enc, 0, case.n), checks, "after the poison was removed")
    enc.close(); dec.close()


@pytest.mark.gpu
def test_argument_checks_on_a_live_handle(gpu, cases):
    from cool_chic_amd._lib import lib

    L = lib()
    case = cases["odd18x65"][0]
    enc = gpu(0)
    h = enc._h
    dev = C.c_void_p()
    assert L.ccd_enc_measure_deltas(h, None) == 0 and L.ccd_enc_wait(h, None) == 0  # an empty handle measures nothing
    enc.add(case.arch, case.nn, case.latents)
    assert L.ccd_enc_slot_delta_map(h, 0, 0, C.byref(dev)) == ERR_ARG  # before any deltas call
    enc.measure(rate_map=True); enc.wait()
    assert L.ccd_enc_slot_delta_map(h, 0, 0, C.byref(dev)) == ERR_ARG and not dev.value  # a measure is not a deltas call
    enc.measure_deltas(); enc.wait()
    assert L.ccd_enc_slot_delta_map(h, 0, 0, C.byref(dev)) == case.hw[0][0] * case.hw[0][1] and dev.value
    for grid in (-1, case.n):
        assert L.ccd_enc_slot_delta_map(h, 0, grid, C.byref(dev)) == ERR_ARG
    for slot in (-1, 1):
        assert L.ccd_enc_slot_delta_map(h, slot, 0, C.byref(dev)) == ERR_ARG
    assert L.ccd_enc_slot_delta_map(h, 0, 0, None) == ERR_ARG
    want = _words(_maps(enc, 0, case.n))
    enc.run(); enc.wait()  # a run leaves the maps alone
    assert _words(_maps(enc, 0, case.n)) == want
    # a second call while one is in flight: what measure does in that state - the first is waited for, the call succeeds
    assert L.ccd_enc_measure(h, None, 0) == 0 and L.ccd_enc_measure(h, None, 0) == 0 and L.ccd_enc_wait(h, None) == 0
    assert L.ccd_enc_slot_delta_map(h, 0, 0, C.byref(dev)) == ERR_ARG  # the last measure was not a deltas call
    assert L.ccd_enc_measure_deltas(h, None) == 0 and L.ccd_enc_measure_deltas(h, None) == 0 and L.ccd_enc_wait(h, None) == 0
    assert _words(_maps(enc, 0, case.n)) == want
    enc.add(case.arch, case.nn, case.latents)  # a slot no deltas call covered yet
    assert L.ccd_enc_slot_delta_map(h, 1, 0, C.byref(dev)) == ERR_ARG
    enc.measure_deltas(); enc.wait()
    assert _words(_maps(enc, 1, case.n)) == want
    enc.close()


@pytest.mark.gpu
def test_rd_evaluator(gpu, oracle, cases):
    from cool_chic_amd import RdEvaluator
    from cool_chic_amd.quality import _planes_to_frame_data

    case, checks = cases["odd100x37"]
    dec = _decoded(["odd100x37"], oracle, bitdepth=8)
    source = _planes_to_frame_data(dec.planes(0), 8, "rgb")
    ev = RdEvaluator(0)
    ev.add(case.arch, case.nn, case.latents, source)
    lat2 = [a.copy() for a in case.latents]
    lat2[0][5, 5] += 1 if lat2[0][5, 5] < 63 else -1
    ev.add(case.arch, case.nn, lat2, source)
    plain = ev.evaluate(1e-3)
    with_maps = ev.evaluate(1e-3, rate_deltas=True)
    assert len(plain) == len(with_maps) == 2
    for a, b in zip(plain, with_maps):
        assert _bits64(a.rate) == _bits64(b.rate) and a.rate.status == b.rate.status == 0
        assert a.rate.sum_width.tolist() == b.rate.sum_width.tolist() and a.rate.n_symbols.tolist() == b.rate.n_symbols.tolist()
        assert a.rate[4:] == b.rate[4:] and (a.mse, a.bits, a.cost) == (b.mse, b.bits, b.cost)
        for f in ("bitdepth", "frame_data_type", "sse", "n", "n_scales", "cs", "ssim"):
            assert getattr(a.quality, f) == getattr(b.quality, f), f
    m, y, x, sign, ref = next(c for c in checks if c[0] == 1 and case.n_dep(*c[:3]) > case.n_sp)
    import torch

    mp = torch.as_tensor(ev.rate_delta_map(0, m), device="cuda").cpu().numpy()
    assert mp.shape == (2,) + case.hw[m] and mp.dtype == np.float32
    dev = float(mp[(sign + 1) // 2, y, x])
    assert abs(dev - ref) <= case.bound(m, y, x, ref), (dev, ref)
    ev.close(); dec.close()


@pytest.mark.gpu
def test_cross_check_against_the_meter_on_kodim14(gpu, oracle):
    """Not the primary reference: 64 perturbed candidates of kodim14 through the EXISTING meter, measure()'s total_bits minus the
    base's against the map, same bound.  Reaches the 64 x 64 dependent blocks of the coarsest grids."""
    hdr, nn, lat = _cool_chics(oracle, load_golden("kodim14")[0])[0]
    case = _Case(oracle, "kodim14", hdr, nn, lat, planes=False)  # the oracle's bit planes of kodim14 are not needed here
    nn, base_lat = case.nn, case.latents
    rng = np.random.default_rng(14)
    triples = []
    for _ in range(64):
        m = int(rng.integers(case.n))
        y, x = int(rng.integers(case.hw[m][0])), int(rng.integers(case.hw[m][1]))
        s = int(rng.choice([-1, 1]))
        if not -64 <= int(base_lat[m][y, x]) + s <= 63:
            s = -s
        triples.append((m, y, x, s))
    assert max(len(rw) for m, y, x, _ in triples for _, rw, _ in case.ifce_blocks(m, y, x)) >= 64
    enc = gpu(0)
    enc.add(case.arch, nn, base_lat)
    for m, y, x, s in triples:
        lat2 = list(base_lat)
        lat2[m] = base_lat[m].copy()
        lat2[m][y, x] += s
        enc.add(case.arch, nn, lat2)
    enc.measure(); enc.wait()
    totals = [enc.rate(k).total_bits for k in range(65)]
    alone = gpu(0)
    alone.add(case.arch, nn, base_lat)
    alone.measure_deltas(); alone.wait()
    maps = _maps(alone, 0, case.n)
    assert _bits64(alone.rate(0)) == _bits64(enc.rate(0))
    alone.close(); enc.close()
    worst = 0.0
    for k, (m, y, x, s) in enumerate(triples):
        ref = totals[k + 1] - totals[0]
        dev = float(maps[m][(s + 1) // 2, y, x])
        bound = case.bound(m, y, x, ref)
        print(f"kodim14 grid {m} ({y}, {x}) {s:+d}: map {dev!r} meter {ref!r} |diff| {abs(dev - ref):.3g} bound {bound:.3g} deps {case.n_dep(m, y, x)}")
        worst = max(worst, abs(dev - ref) / bound)
    print(f"kodim14 cross-check: worst deviation {worst:.3g} of the bound")
    for k, (m, y, x, s) in enumerate(triples):
        ref = totals[k + 1] - totals[0]
        assert abs(float(maps[m][(s + 1) // 2, y, x]) - ref) <= case.bound(m, y, x, ref), (m, y, x, s)
