"""ARM parameter deltas (ccd_enc_measure_param_deltas, EncodeBatch.measure_param_deltas / param_deltas, nnrefine.ArmRefiner;
DESIGN.md section 4.20): for every transmitted integer of a cool-chic's ARM the exact change of the slot's model bits, of its
sum of interval widths and the number of symbols whose width changed, if that one integer were v - 1 or v + 1.

The reference is the CPU oracle, built as tests/test_rate_deltas.py builds it: values +- 1 go through writer.encode_network and
writer.encode_coolchic, oracle.decode_coolchic(stop_after_entropy=True) decodes the bytes, oracle.laplace_bounds gives every
interval, numpy float64 every pixel's 24 - log2(width), and ONE math.fsum runs over the pixels whose bits differ.

Bounds: |dev - ref| <= 2 * moved_ref * TERM_TOL for `bits` (TERM_TOL = 24 * 2^-48, the project's bound per log2 term; two
logarithms per moved pixel), exactly 0.0 where nothing moved; `moved` and `sum_width` equal the reference exactly.

The oracle tests run in mode 0, which is the incremental path wherever a slot's state fits the LDS (all cases but
arm_s40_i31_h7); test_modes compares its words with the generic path's."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import arm_layouts
from conftest import ROOT, load_golden
from test_rate_deltas import _WIDTH, _cool_chics

ERR_VALUE, ERR_UNSUPPORTED, ERR_ARG = -2, -4, -7
ENTRY_POINTS = ["ccd_enc_measure_param_deltas", "ccd_enc_slot_param_count", "ccd_enc_slot_param_deltas"]
TERM_TOL = 24.0 * 2.0 ** -48
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


# ---- CPU -------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_refuse_null():
    import cool_chic_amd
    from cool_chic_amd import _lib, nnrefine
    from cool_chic_amd.encoder import EncodeBatch

    with open(os.path.join(ROOT, "include", "ccd.h")) as f:
        header = f.read()
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert name + "(" in header, name
        assert name in _lib.SIGNATURES, name
        assert getattr(L, name) is not None
    assert all(hasattr(EncodeBatch, m) for m in ("measure_param_deltas", "param_deltas", "param_count"))
    for name in ("ArmRefiner", "expgol_bit_deltas", "pick_moves", "ParamDeltas"):
        assert getattr(cool_chic_amd, name) is not None
    assert cool_chic_amd.ArmRefiner is nnrefine.ArmRefiner
    # NULL arguments: argument errors without a device
    first, count = C.c_int(7), C.c_int(7)
    assert L.ccd_enc_measure_param_deltas(None, None, 0, -1, 0) == ERR_ARG
    assert L.ccd_enc_slot_param_count(None, 0) == ERR_ARG
    assert L.ccd_enc_slot_param_deltas(None, 0, C.byref(first), C.byref(count), None, None, None) == ERR_ARG
    assert (first.value, count.value) == (7, 7)


def _first_coolchic(oracle, name):
    from cool_chic_amd import writer

    hdr, nn, lat = _cool_chics(oracle, load_golden(name)[0])[0]
    arch = writer.parse_cc_header(hdr)
    return arch, nn, lat, writer.network_values(arch, nn)


@pytest.mark.parametrize("name", ["odd18x65", "odd100x37", "vid3_ldp"])
def test_expgol_bit_deltas_are_the_payloads_change(oracle, name):
    from cool_chic_amd import writer
    from cool_chic_amd._lib import CCHeader
    from cool_chic_amd.nnrefine import build_candidate, expgol_bit_deltas, payload_byte_deltas

    arch, nn, _, values = _first_coolchic(oracle, name)
    n_arm = sum(writer.network_layout(arch)[:2])

    def payload_bits(v):
        h = CCHeader.from_buffer_copy(bytes(arch))
        return 8 * len(writer.encode_network(h, v)) - h.nn_n_bit_pad

    base = payload_bits(values)
    assert base == 8 * len(nn) - arch.nn_n_bit_pad
    table = expgol_bit_deltas(arch, values)
    assert table.shape == (n_arm, 2) and table.dtype == np.float64
    h0, nn0 = build_candidate(arch, values)
    rechosen = payload_byte_deltas(arch, values)
    for k in range(n_arm):
        for j, s in enumerate((-1, 1)):
            v = values.copy()
            v[k] += s
            assert table[k, j] == payload_bits(v) - base, (k, s)
            if name == "odd100x37":  # the refiner's own table: bytes with every order chosen again
                assert rechosen[k, j] == 8 * (len(build_candidate(arch, v)[1]) - len(nn0)), (k, s)
    # the int32 edges: a move that cannot be transmitted
    v = values.copy()
    v[0], v[n_arm - 1] = INT32_MAX, INT32_MIN
    for t in (expgol_bit_deltas(arch, v), payload_byte_deltas(arch, v)):
        assert t[0, 1] == np.inf and t[n_arm - 1, 0] == np.inf and np.isfinite(t[0, 0]) and np.isfinite(t[n_arm - 1, 1])
        assert np.isinf(t).sum() == 2
    with pytest.raises(ValueError):
        expgol_bit_deltas(arch, values[:-1])


def test_pick_moves_against_enumeration():
    from cool_chic_amd.nnrefine import pick_moves

    def enumerate_moves(a, b, max_moves):
        best = []
        for k in range(a.shape[0]):
            cands = [(float(a[k, j] + b[k, j]), k, s) for j, s in enumerate((-1, 1)) if a[k, j] + b[k, j] < 0]
            if cands:
                best.append(min(cands))
        return sorted(best)[:max_moves]

    rng = np.random.default_rng(20)
    n_ties = n_inf = 0
    for trial in range(200):
        n = int(rng.integers(1, 40))
        a = rng.integers(-6, 7, size=(n, 2)).astype(np.float64) * 0.5  # few distinct values: ties between parameters and signs
        b = rng.integers(-2, 3, size=(n, 2)).astype(np.float64) * 8.0
        if trial % 3 == 0:
            a[rng.random((n, 2)) < 0.2] = np.inf
        if trial % 7 == 0:
            a, b = np.abs(a), np.abs(b)  # nothing promises a gain
        for max_moves in (0, 1, 3, n, n + 5):
            got = pick_moves(a, b, max_moves)
            want = enumerate_moves(a, b, max_moves)
            assert [(m.delta, m.index, m.sign) for m in got] == want
            assert len({m.index for m in got}) == len(got) <= max_moves and all(m.delta < 0 for m in got)
        t = a + b
        n_ties += int(((t[:, 0] == t[:, 1]) & (t[:, 0] < 0)).sum())
        n_inf += int(np.isinf(t).sum())
        if trial % 7 == 0:
            assert pick_moves(a, b, n) == []
    assert n_ties > 20 and n_inf > 50  # the made-up tables do hold ties between the signs and moves that do not exist
    tie = np.array([[-1.0, -1.0], [-1.0, 0.0], [0.0, -1.0], [np.inf, -2.0], [np.inf, np.inf]])
    assert [(m.index, m.sign) for m in pick_moves(tie, np.zeros_like(tie), 9)] == [(3, 1), (0, -1), (1, -1), (2, 1)]
    with pytest.raises(ValueError):
        pick_moves(np.zeros((3, 3)), np.zeros((3, 3)), 1)


# ---- the reference ---------------------------------------------------------------------------------------------------
def _width_planes(oracle, hdr, nn, lat):
    """([int8 (h, w)] latents, [int64 (h, w)] right - left of every latent's interval, raster): test_rate_deltas._bit_planes
    before its logarithm, sharing its cache of oracle.laplace_bounds."""
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
        planes.append(width.reshape(h, w))
    return [np.ascontiguousarray(a) for a in r["latent"]], planes


class _ParamCase:
    """One cool-chic: architecture, network integers, latents, the base widths; reference(k, sign) from the oracle."""

    def __init__(self, oracle, name, hdr, nn, lat, values=None):
        from cool_chic_amd import writer
        from cool_chic_amd._lib import CCHeader

        self.name, self.oracle = name, oracle
        self.arch = writer.parse_cc_header(hdr)
        if values is None:
            self.nn, self.values = nn, writer.network_values(self.arch, nn)
            self.latents, self.base = _width_planes(oracle, hdr, nn, lat)
        else:  # other integers in the same architecture, over the same latents
            self.latents = [np.ascontiguousarray(a) for a in oracle.decode_coolchic(hdr, nn, lat, stop_after_entropy=True)["latent"]]
            self.values = np.asarray(values, np.int32).copy()
            self.arch = CCHeader.from_buffer_copy(bytes(self.arch))
            self.nn = writer.encode_network(self.arch, self.values)
            got, self.base = self._planes(self.values)
            assert all(np.array_equal(a, b) for a, b in zip(got, self.latents))
        self.base_bits = [24.0 - np.log2(w.astype(np.float64)) for w in self.base]
        self.layout = writer.network_layout(self.arch)
        self.n_w, self.n_arm = self.layout[0], self.layout[0] + self.layout[1]
        self.dim, self.n_layers = int(self.arch.total_context_arm), int(self.arch.n_hidden_layers_arm) + 1
        self.n_symbols = sum(int(w.size) for w in self.base)
        self.n_decodes = 0
        self._refs = {}

    def _planes(self, values):
        from cool_chic_amd import writer
        from cool_chic_amd._lib import CCHeader

        h = CCHeader.from_buffer_copy(bytes(self.arch))
        nn = writer.encode_network(h, values)
        cc = writer.encode_coolchic(h, nn, self.latents)
        h2 = writer.parse_cc_header(cc)
        p, q = h2.n_bytes_header, h2.n_bytes_header + h2.nn_n_bytes
        assert cc[p:q] == nn
        return _width_planes(self.oracle, cc[:p], cc[p:q], cc[q:])

    def total_bits(self):
        return math.fsum(v for b in self.base_bits for v in b.ravel().tolist())

    def reference(self, k, sign):
        """(bits, sum_width, moved) of values[k] + sign against the base; one fsum over the pixels whose bits differ."""
        if (k, sign) not in self._refs:
            v = self.values.copy()
            v[k] += sign
            got, planes = self._planes(v)
            assert all(np.array_equal(a, b) for a, b in zip(got, self.latents))
            self.n_decodes += 1
            terms, d_width, moved = [], 0, 0
            for new, old, old_bits in zip(planes, self.base, self.base_bits):
                idx = new != old
                terms += (24.0 - np.log2(new[idx].astype(np.float64))).tolist() + (-old_bits[idx]).tolist()
                d_width += int(new[idx].sum()) - int(old[idx].sum())
                moved += int(idx.sum())
            self._refs[(k, sign)] = (math.fsum(terms), d_width, moved)
        return self._refs[(k, sign)]

    def layer_firsts(self):
        """First weight of every layer (hidden layers, the output layer, then the stabiliser when it is transmitted)."""
        d = self.dim
        out = [l * d * d for l in range(self.n_layers)]
        if self.arch.linear_stabiliser_arm:
            out.append((self.n_layers - 1) * d * d + 2 * d)
        return out


def _check(case, table, pairs, what):
    """Rows of a ParamDeltas against the oracle for [(k, sign)]; returns the largest |dev - ref| / bound."""
    worst = 0.0
    for k, sign in pairs:
        ref_bits, ref_width, ref_moved = case.reference(k, sign)
        r, j = k - table.first, (sign + 1) // 2
        assert 0 <= r < table.bits.shape[0], (what, case.name, k, table.first, table.bits.shape)
        dev = float(table.bits[r, j])
        assert int(table.moved[r, j]) == ref_moved and int(table.sum_width[r, j]) == ref_width, \
            (what, case.name, k, sign, int(table.moved[r, j]), ref_moved, int(table.sum_width[r, j]), ref_width)
        if ref_moved == 0:
            assert dev == 0.0 and not np.signbit(dev), (what, case.name, k, sign, dev)
            continue
        bound = 2.0 * ref_moved * TERM_TOL
        err = abs(dev - ref_bits)
        worst = max(worst, err / bound)
        assert err <= bound, (what, case.name, k, sign, dev, ref_bits, err, bound)
    return worst


def _shape_ok(table, first, count):
    assert table.first == first and table.bits.shape == table.sum_width.shape == table.moved.shape == (count, 2)
    assert table.bits.dtype == np.float64 and table.sum_width.dtype == np.int64 and table.moved.dtype == np.int64
    assert not np.isnan(table.bits).any() and not (table.bits == -np.inf).any()


def _words(table):
    return (table.first, table.bits.view(np.uint64).tolist(), table.sum_width.tolist(), table.moved.tolist())


# ---- GPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cool_chic_amd import EncodeBatch, _lib

    _lib.lib()
    return EncodeBatch


def _table(gpu, case, first=0, count=-1, mode=0):
    enc = gpu(0)
    try:
        enc.add(case.arch, case.nn, case.latents)
        enc.measure_param_deltas(first=first, count=count, mode=mode)
        enc.wait()
        return enc.param_deltas(0)
    finally:
        enc.close()


@pytest.fixture(scope="module")
def small(oracle):
    """odd18x65 and odd100x37, first cool-chic: the cases; their 360 references each are made when first asked for and kept."""
    return {name: _ParamCase(oracle, name, *_cool_chics(oracle, load_golden(name)[0])[0]) for name in ("odd18x65", "odd100x37")}


def _all_pairs(case):
    return [(k, s) for k in range(case.n_arm) for s in (-1, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["odd18x65", "odd100x37"])
def test_whole_table_against_the_oracle(gpu, small, name):
    case = small[name]
    assert case.n_arm == 180 and case.dim == 8 and case.n_layers == 3 and case.arch.linear_stabiliser_arm
    table = _table(gpu, case)
    _shape_ok(table, 0, case.n_arm)
    assert np.isfinite(table.bits).all()
    worst = _check(case, table, _all_pairs(case), "whole table")
    still = [(k, s) for k, s in _all_pairs(case) if case.reference(k, s)[2] == 0]
    if name == "odd100x37":  # a parameter no pixel answers to: exactly 0.0, 0, 0
        assert still, "no entry with moved == 0"
    print(f"{name}: {2 * case.n_arm} candidates, {case.n_decodes} oracle decodes, {len(still)} move nothing {still[:6]}, "
          f"worst deviation {worst:.3g} of the bound")


@pytest.mark.gpu
def test_sampled_table_against_the_oracle_vid3_ldp(gpu, oracle):
    case = _ParamCase(oracle, "vid3_ldp", *_cool_chics(oracle, load_golden("vid3_ldp")[0])[0])
    rng = np.random.default_rng(4321)
    d, firsts = case.dim, case.layer_firsts()
    must = []
    for i, f in enumerate(firsts):  # first and last weight of every layer; the stabiliser: both rows
        last = (firsts[i + 1] if i + 1 < len(firsts) else case.n_w) - 1
        must += [f, last]
    if case.arch.linear_stabiliser_arm:
        must += [firsts[-1] + d - 1, firsts[-1] + d]
        must += [case.n_arm - 2, case.n_arm - 1]  # the stabiliser's biases
    must += [case.n_w, case.n_arm - 1]            # first and last bias
    must = list(dict.fromkeys(must))
    rest = [k for k in range(case.n_arm) if k not in set(must)]
    picks = must + [rest[i] for i in rng.choice(len(rest), size=48, replace=False)]
    table = _table(gpu, case)
    _shape_ok(table, 0, case.n_arm)
    worst = _check(case, table, [(k, s) for k in picks for s in (-1, 1)], "sampled table")
    assert case.n_decodes <= 140, case.n_decodes
    print(f"vid3_ldp: dim {d}, {case.n_layers} layers, {case.n_arm} ARM integers, {case.n_decodes} oracle decodes, "
          f"worst deviation {worst:.3g} of the bound")


LAYOUT_NAMES = (["arm_s%d_i%d_h%d" % s for s in arm_layouts.ARM_SHAPES] +
                ["ifce0_15_18x65_s%d_i%d_h%d" % s for s in arm_layouts.PLACEMENT_SHAPES] +
                ["tiny%dx%d_s%d_i%d_h%d" % (size + shape) for size in ((1, 1), (1, 29), (5, 34)) for shape, _ in arm_layouts.TINY_SHAPES])
_LAYOUTS = {}


def _layout(name):
    """A case of tests/arm_layouts.py, made once; all of them only when something else has made them already."""
    if name not in _LAYOUTS:
        if arm_layouts._CASES is not None:
            _LAYOUTS[name] = arm_layouts.case(name)
        else:
            _LAYOUTS[name] = arm_layouts.make_case(next(s for s in arm_layouts.specs() if s[0] == name))
    return _LAYOUTS[name]


def _layout_ranges(case):
    """[(first, count)] of at most 8 parameters: around every layer boundary, around the stabiliser, at both ends of the biases."""
    marks = case.layer_firsts()[1:] + [case.n_w, case.n_arm]  # a range straddles each mark; the first range starts at 0
    out = [(0, min(8, case.n_arm))]
    for m in marks:
        first = max(m - 4, 0)
        out.append((first, min(8, case.n_arm - first)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", LAYOUT_NAMES)
def test_layouts(gpu, oracle, name):
    c = _layout(name)
    case = _ParamCase(oracle, name, c.hdr, c.nn, c.payload)
    assert case.dim == c.shape[0] + c.shape[1] and case.n_layers == c.shape[2] + 1
    ranges = _layout_ranges(case)
    # the oracle's share: the two parameters on either side of every mark and both ends of the ARM, both signs while 64 decodes
    # allow it, else alternating signs
    picks = sorted({k for first, count in ranges for k in (first + count // 2 - 1, first + count // 2) if first <= k < first + count} |
                   {0, case.n_arm - 1})
    both = 2 * len(picks) <= 64
    pairs = [(k, s) for i, k in enumerate(picks) for s in ((-1, 1) if both else ((-1,) if i % 2 else (1,)))]
    enc = gpu(0)
    enc.add(case.arch, case.nn, case.latents)
    assert enc.param_count(0) == case.n_arm
    worst, seen = 0.0, set()
    for first, count in ranges:
        assert count <= 8
        enc.measure_param_deltas(first=first, count=count)
        enc.wait()
        table = enc.param_deltas(0)
        _shape_ok(table, first, count)
        mine = [(k, s) for k, s in pairs if first <= k < first + count]
        worst = max(worst, _check(case, table, mine, "layout"))
        seen |= set(mine)
    enc.close()
    assert seen == set(pairs) and case.n_decodes <= 64, (case.n_decodes, len(pairs))
    print(f"{name}: dim {case.dim}, {case.n_layers} layers, {case.n_arm} ARM integers, {len(ranges)} ranges, {case.n_decodes} oracle "
          f"decodes, worst deviation {worst:.3g} of the bound")


MODE_LAYOUTS = ["tiny1x1_s5_i2_h1", "tiny1x29_s6_i0_h2", "tiny5x34_s5_i2_h1", "tiny5x34_s6_i0_h2", "arm_s1_i0_h0", "arm_s39_i31_h0",
                "arm_s3_i2_h4", "arm_s2_i7_h5", "ifce0_15_18x65_s6_i3_h3", "ifce0_15_18x65_s9_i7_h6", "arm_s40_i25_h1", "arm_s40_i24_h2"]


@pytest.mark.gpu
def test_modes(gpu, oracle, small):
    """mode 1 (generic) and mode 2 (incremental) give the same words: the three reference fixtures, whole table, and layouts with
    0 .. 6 hidden layers (no hidden layer, the output layer next, one layer behind the next, the tail recomputed in full through
    the scratch columns), every range test_layouts asks for.  mode 0 gives those words too.  arm_s40_i31_h7's state (10 x 71
    columns per lane) does not fit the LDS: mode 2 is CCD_ERR_UNSUPPORTED before any device work, the handle stays usable and
    mode 0 gives mode 1's words there."""
    from cool_chic_amd._lib import CcdError, lib

    cases = [(small["odd18x65"], [(0, -1)]), (small["odd100x37"], [(0, -1)]),
             (_ParamCase(oracle, "vid3_ldp", *_cool_chics(oracle, load_golden("vid3_ldp")[0])[0]), [(0, -1)])]
    for name in MODE_LAYOUTS:
        c = _layout(name)
        case = _ParamCase(oracle, name, c.hdr, c.nn, c.payload)
        cases.append((case, [(0, -1)] if case.n_arm <= 512 else _layout_ranges(case)))
    n_moved = 0
    for case, ranges in cases:
        enc = gpu(0)
        enc.add(case.arch, case.nn, case.latents)
        for first, count in ranges:
            words = {}
            for mode in (1, 2, 0):
                enc.measure_param_deltas(first=first, count=count, mode=mode); enc.wait()
                t = enc.param_deltas(0)
                words[mode] = _words(t)
                n_moved += int((t.moved > 0).sum()) if mode == 2 else 0
            assert words[2] == words[1], (case.name, first, count)
            assert words[0] == words[1], (case.name, first, count)
        enc.close()
    assert n_moved > 1000  # the comparison is not one of empty tables
    wide = _layout("arm_s40_i31_h7")
    case = _ParamCase(oracle, wide.name, wide.hdr, wide.nn, wide.payload)
    enc = gpu(0)
    enc.add(case.arch, case.nn, case.latents)
    enc.measure_param_deltas(count=16, mode=1); enc.wait()
    generic, rate = _words(enc.param_deltas(0)), enc.rate(0)
    with pytest.raises(CcdError) as e:
        enc.measure_param_deltas(count=16, mode=2)
    assert e.value.code == ERR_UNSUPPORTED
    # refused before the device was touched: nothing is in flight, the last table and the meter's results stand
    assert lib().ccd_enc_wait(enc._h, None) == 0
    assert _words(enc.param_deltas(0)) == generic and enc.rate(0).total_bits == rate.total_bits
    enc.measure_param_deltas(count=16, mode=0); enc.wait()
    assert _words(enc.param_deltas(0)) == generic
    for kwargs in (dict(mode=3), dict(mode=-1), dict(first=-1)):
        with pytest.raises(CcdError) as e:
            enc.measure_param_deltas(**kwargs)
        assert e.value.code == ERR_ARG
    assert _words(enc.param_deltas(0)) == generic  # refusals leave the table alone
    # a batch of both kinds: mode 0 prices each slot by its own path, mode 2 refuses the call for the one that does not fit
    other = small["odd100x37"]
    enc.add(other.arch, other.nn, other.latents)
    enc.measure_param_deltas(count=16, mode=0); enc.wait()
    assert _words(enc.param_deltas(0)) == generic
    mixed = _words(enc.param_deltas(1))
    with pytest.raises(CcdError) as e:
        enc.measure_param_deltas(count=16, mode=2)
    assert e.value.code == ERR_UNSUPPORTED
    enc.measure_param_deltas(count=16, mode=1); enc.wait()
    assert _words(enc.param_deltas(1)) == mixed and _words(enc.param_deltas(0)) == generic
    enc.close()


@pytest.mark.gpu
def test_a_slot_gives_the_same_words_alone_in_a_batch_twice_and_by_range(gpu, oracle, small):
    from cool_chic_amd import writer

    case = small["odd100x37"]
    alone = gpu(0)
    alone.add(case.arch, case.nn, case.latents)
    alone.measure_param_deltas(); alone.wait()
    full = alone.param_deltas(0)
    want = _words(full)
    alone.measure_param_deltas(); alone.wait()  # a second call
    assert _words(alone.param_deltas(0)) == want
    for first, count in ((0, 1), (3, 64), (37, 65), (100, 80), (179, 1), (179, 5), (60, -1)):  # sub-ranges: rows of the full table
        alone.measure_param_deltas(first=first, count=count); alone.wait()
        t = alone.param_deltas(0)
        n = min(count if count >= 0 else case.n_arm, case.n_arm - first)
        _shape_ok(t, first, n)
        assert t.bits.view(np.uint64).tolist() == full.bits[first:first + n].view(np.uint64).tolist(), (first, count)
        assert np.array_equal(t.sum_width, full.sum_width[first:first + n]) and np.array_equal(t.moved, full.moved[first:first + n])
    alone.measure_param_deltas(first=500, count=4); alone.wait()  # a range past the slot's parameters: clipped to nothing
    _shape_ok(alone.param_deltas(0), case.n_arm, 0)
    alone.close()
    # behind two slots of other architectures (kodim14: 20 contexts, 924 ARM integers, clipped to the first 180; rgb192)
    mixed = gpu(0)
    for name in ("kodim14", "rgb192"):
        hdr, nn, lat = _cool_chics(oracle, load_golden(name)[0])[0]
        mixed.add(writer.parse_cc_header(hdr), nn, oracle.decode_coolchic(hdr, nn, lat, stop_after_entropy=True)["latent"])
    assert mixed.add(case.arch, case.nn, case.latents) == 2
    mixed.measure_param_deltas(count=180); mixed.wait()
    assert _words(mixed.param_deltas(2)) == want
    assert mixed.param_deltas(0).bits.shape == (180, 2) and mixed.param_count(0) > 180
    mixed.close()


@pytest.mark.gpu
def test_meter_and_writer_are_untouched(gpu, small):
    from cool_chic_amd._lib import CcdError

    case = small["odd18x65"]
    enc = gpu(0)
    enc.add(case.arch, case.nn, case.latents)
    enc.run(); enc.wait()
    before = enc.bytes(0)
    enc.measure(); enc.wait()
    plain = enc.rate(0)
    enc.measure_param_deltas(); enc.wait()
    r = enc.rate(0)
    assert r.status == plain.status == 0
    assert np.concatenate([r.bits, [r.total_bits]]).view(np.uint64).tolist() == np.concatenate([plain.bits, [plain.total_bits]]).view(np.uint64).tolist()
    assert r.sum_width.tolist() == plain.sum_width.tolist() and r.n_symbols.tolist() == plain.n_symbols.tolist()
    assert (r.n_bytes_nn, r.n_bytes_header) == (plain.n_bytes_nn, plain.n_bytes_header)
    for call in (lambda: enc.delta_map(0, 0), lambda: enc.rate_map(0, 0)):  # as after a plain measure
        with pytest.raises(CcdError) as e:
            call()
        assert e.value.code == ERR_ARG
    want = _words(enc.param_deltas(0))
    enc.run(); enc.wait()  # a run leaves the table alone and writes the bytes it wrote before
    assert enc.bytes(0) == before and _words(enc.param_deltas(0)) == want
    enc.measure(); enc.wait()  # the next measure of any kind invalidates it
    with pytest.raises(CcdError) as e:
        enc.param_deltas(0)
    assert e.value.code == ERR_ARG
    enc.measure_deltas(); enc.wait()
    with pytest.raises(CcdError):
        enc.param_deltas(0)
    enc.close()


@pytest.mark.gpu
def test_poisoned_device_latent_is_that_slots_error_only(gpu, oracle, small):
    import torch

    from cool_chic_amd._lib import CcdError
    from test_rate_deltas import _decoded, _device_grid

    names = ["odd18x65", "odd18x65", "odd100x37"]
    dec = _decoded(names, oracle)
    plane = _device_grid(dec, 1, 0)
    plane[3, 5] = 64
    torch.cuda.synchronize()
    enc = gpu(0)
    for s in range(3):
        enc.add_from_decode(dec, s)
    enc.measure_param_deltas()
    with pytest.raises(CcdError) as e:
        enc.wait()
    assert e.value.code == ERR_VALUE
    assert enc.rate(1).status == ERR_VALUE
    with pytest.raises(CcdError) as e:
        enc.param_deltas(1)
    assert e.value.code == ERR_VALUE
    for s in (0, 2):
        case = small[names[s]]
        assert enc.rate(s).status == 0
        _check(case, enc.param_deltas(s), _all_pairs(case), "beside a poisoned slot")
    enc.close(); dec.close()


@pytest.mark.gpu
def test_int32_edges(gpu, oracle):
    c = _layout("tiny1x29_s5_i2_h1")
    base = _ParamCase(oracle, c.name, c.hdr, c.nn, c.payload)
    values = base.values.copy()
    k_w, k_b = 3, base.n_w + 1  # a weight of the first layer, a bias of the first layer
    values[k_w], values[k_b] = INT32_MAX, INT32_MIN
    case = _ParamCase(oracle, c.name + " at the int32 edges", c.hdr, c.nn, c.payload, values=values)
    table = _table(gpu, case)
    _shape_ok(table, 0, case.n_arm)
    for k, j in ((k_w, 1), (k_b, 0)):
        assert table.bits[k, j] == np.inf and table.sum_width[k, j] == 0 and table.moved[k, j] == 0
    assert np.isinf(table.bits).sum() == 2
    pairs = [(k_w, -1), (k_b, 1)] + [(k, s) for k in (k_w - 1, k_w + 1, k_b - 1, k_b + 1, 0, case.n_arm - 1) for s in (-1, 1)]
    worst = _check(case, table, pairs, "int32 edges")
    print(f"int32 edges: {len(pairs)} pairs, worst deviation {worst:.3g} of the bound")


# ---- the refiner -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refined(gpu, oracle, small):
    """odd100x37's device latents and the two descents: (case, decode batch, pointers, batch=1 result, batch=8 result)."""
    from cool_chic_amd import ArmRefiner
    from cool_chic_amd._lib import lib
    from test_rate_deltas import _decoded

    case = small["odd100x37"]
    dec = _decoded(["odd100x37"], oracle)
    ptrs = [lib().ccd_batch_latent(dec._h, 0, g) for g in range(dec.header(0).n_grids)]
    one = ArmRefiner(0).refine(case.arch, case.values, ptrs, max_steps=25, batch=1, owner=dec)
    eight = ArmRefiner(0).refine(case.arch, case.values, ptrs, max_steps=25, batch=8, owner=dec)
    yield case, dec, ptrs, one, eight
    dec.close()


def _oracle_total(case, header, nn):
    """(latents, total bits as one fsum) of the stream the host writer makes of a network over the case's latents."""
    from cool_chic_amd import writer

    cc = writer.encode_coolchic(header, nn, case.latents)
    h2 = writer.parse_cc_header(cc)
    p, q = h2.n_bytes_header, h2.n_bytes_header + h2.nn_n_bytes
    assert cc[p:q] == nn
    lat, widths = _width_planes(case.oracle, cc[:p], cc[p:q], cc[q:])
    return lat, math.fsum(v for w in widths for v in (24.0 - np.log2(w.astype(np.float64))).ravel().tolist())


@pytest.mark.gpu
def test_refiner_single_moves(refined):
    from cool_chic_amd.nnrefine import build_candidate, payload_byte_deltas

    case, _, _, res, _ = refined
    assert res.log and len(res.log) <= 25
    # the best single move by exhaustive enumeration on the CPU, orders chosen again for every candidate (the refiner's rule)
    base_total = case.total_bits()
    _, nn0 = build_candidate(case.arch, case.values)
    best = None
    for k, s in _all_pairs(case):
        v = case.values.copy()
        v[k] += s
        d_bits, _, moved = case.reference(k, s)
        key = (base_total + d_bits + 8.0 * len(build_candidate(case.arch, v)[1]), k, s, moved)
        if best is None or key < best:
            best = key
    first = res.log[0]
    print(f"start {res.start_objective!r} (CPU {base_total + 8.0 * len(nn0)!r}); best single move on the CPU: parameter {best[1]} at {best[2]:+d}, "
          f"{best[0]!r}; the refiner's first step: {[(m.index, m.sign) for m in first.moves]}, {first.objective!r}")
    assert abs(first.objective - best[0]) <= 2.0 * best[3] * TERM_TOL, (first.objective, best)
    assert [(m.index, m.sign) for m in first.moves] == [(best[1], best[2])] and not first.rejected
    # every step: strictly below the one before, predicted == true within the bound, the payload's bytes add exactly
    objective, values, header, nn = res.start_objective, case.values.copy(), *build_candidate(case.arch, case.values)
    for i, step in enumerate(res.log):
        assert step.objective < objective, (i, step.objective, objective)
        assert len(step.moves) == 1
        m = step.moves[0]
        assert abs(step.predicted - step.objective) <= 2.0 * step.moved * TERM_TOL, (i, step.predicted, step.objective, step.moved)
        assert len(nn) + payload_byte_deltas(header, values)[m.index, (m.sign + 1) // 2] / 8.0 == step.n_bytes_nn, i
        assert step.objective == step.total_bits + 8.0 * step.n_bytes_nn
        values[m.index] += m.sign
        header, nn = build_candidate(case.arch, values)
        assert len(nn) == step.n_bytes_nn
        objective = step.objective
    assert np.array_equal(values, res.values) and nn == res.bytes_nn and bytes(header) == bytes(res.header)
    # the returned stream: the same latents in the oracle, and the oracle's bits are the last logged ones (the meter's bound)
    lat, total = _oracle_total(case, res.header, res.bytes_nn)
    assert all(np.array_equal(a, b) for a, b in zip(lat, case.latents))
    assert abs(total - res.log[-1].total_bits) <= case.n_symbols * TERM_TOL, (total, res.log[-1].total_bits)
    print(f"{len(res.log)} steps ({res.stopped}): {res.start_objective:.2f} -> {res.log[-1].objective:.2f} bits, "
          f"network {len(nn0)} -> {len(res.bytes_nn)} bytes")


@pytest.mark.gpu
def test_the_tool_refines_after_the_step_search(gpu, oracle, tmp_path):
    """tools/quantise_networks.py --refine-arm on odd100x37 in a child process: exit 0 (its decode-back assertion inside), the
    refined row costs no more than the searched one at the same PSNR, and the stream it wrote decodes (the oracle)."""
    import re
    import subprocess
    import sys

    bs = load_golden("odd100x37")[0]
    planes = oracle.decode_video(bs)[0]["planes"]
    rng = np.random.default_rng(12)
    noisy = [np.clip(p.astype(np.int64) + rng.integers(-3, 4, p.shape), 0, 255).astype(np.uint8) for p in planes]
    src, inp, out = tmp_path / "source.ppm", tmp_path / "in.cool", tmp_path / "out.cool"
    h, w = noisy[0].shape
    src.write_bytes(b"P6 %d %d 255\n" % (w, h) + np.stack(noisy, axis=-1).tobytes())
    inp.write_bytes(bs)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "quantise_networks.py"), str(inp), str(src), str(out), "--lmbda", "1e-3",
                        "--refine-arm", "3"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0
    rows = {m.group(1): (float(m.group(2)), float(m.group(3)), float(m.group(4)))
            for m in re.finditer(r"^(searched|refined): .* ([0-9.]+) bits, PSNR ([0-9.]+) dB, cost ([0-9.e+-]+)$", r.stdout, re.M)}
    assert set(rows) == {"searched", "refined"} and r.stdout.count("refine 0:") == 1
    assert rows["refined"][1] == rows["searched"][1] and rows["refined"][2] < rows["searched"][2] and rows["refined"][0] < rows["searched"][0]
    back = oracle.decode_video(out.read_bytes())
    assert len(back) == 1 and [p.shape for p in back[0]["planes"]] == [p.shape for p in planes]


@pytest.mark.gpu
def test_refiner_batches_and_backs_off(refined, monkeypatch):
    from cool_chic_amd import ArmRefiner

    case, dec, ptrs, one, eight = refined
    objective = eight.start_objective
    assert eight.start_objective == one.start_objective and eight.log
    for step in eight.log:
        assert step.objective < objective and 1 <= len(step.moves) <= 8
        assert all(true >= before for (_, _, true), before in zip(step.rejected, [objective] * len(step.rejected)))
        objective = step.objective
    assert eight.log[-1].objective <= one.log[0].objective
    lat, total = _oracle_total(case, eight.header, eight.bytes_nn)
    assert all(np.array_equal(a, b) for a, b in zip(lat, case.latents))
    assert abs(total - eight.log[-1].total_bits) <= case.n_symbols * TERM_TOL
    # a made-up table whose batch overshoots: the one good move first, then seven moves that each cost bits but are promised
    # to gain - the batch is halved down to the single move, which is accepted
    refiner = ArmRefiner(0)
    real = refiner._table
    good = one.log[0].moves[0]

    def made_up(h, nn, p, owner, stream):
        bits, t = real(h, nn, p, owner, stream)
        fake = t.bits.copy()
        cost = np.where(np.isfinite(t.bits), t.bits, -np.inf)
        cost[good.index] = -np.inf
        worst = np.argsort(cost.max(axis=1))[::-1][:7]
        assert (cost.max(axis=1)[worst] > 8.0 - good.delta).all()  # each alone outweighs the good move and a byte saved
        fake[good.index, (good.sign + 1) // 2] = -2000.0
        for i, k in enumerate(worst):
            fake[k, int(cost[k].argmax())] = -1000.0 + i
        return bits, t._replace(bits=fake)

    monkeypatch.setattr(refiner, "_table", made_up)
    res = refiner.refine(case.arch, case.values, ptrs, max_steps=1, batch=8, owner=dec)
    assert len(res.log) == 1
    step = res.log[0]
    assert [n for n, _, _ in step.rejected] == [8, 4, 2] and all(true > res.start_objective for _, _, true in step.rejected)
    assert [(m.index, m.sign) for m in step.moves] == [(good.index, good.sign)]
    assert step.objective == one.log[0].objective and step.objective < res.start_objective
    print(f"batch 8: {len(eight.log)} steps to {eight.log[-1].objective:.2f} (batch 1: {len(one.log)} steps to {one.log[-1].objective:.2f}); "
          f"back-off {step.rejected}")
