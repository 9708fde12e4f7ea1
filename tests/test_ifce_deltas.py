"""IFCE parameter deltas (ccd_enc_measure_ifce_deltas, EncodeBatch.measure_ifce_deltas / ifce_deltas, nnrefine.RateRefiner;
DESIGN.md section 4.21): for every transmitted integer of a cool-chic's IFCE the exact change of the slot's model bits, of its
sum of interval widths and the number of symbols whose width changed, if that one integer were v - 1 or v + 1.

The reference is tests/test_param_deltas.py's, built the same way: values +- 1 go through writer.encode_network and
writer.encode_coolchic, oracle.decode_coolchic(stop_after_entropy=True) decodes the bytes, oracle.laplace_bounds gives every
interval, numpy float64 every pixel's 24 - log2(width), and ONE math.fsum runs over the pixels whose bits differ.  IFCE integer k
is values[n_arm + k].

Bounds: |dev - ref| <= 2 * moved_ref * TERM_TOL for `bits` (TERM_TOL = 24 * 2^-48, the project's bound per log2 term; two
logarithms per moved pixel), exactly 0.0 where nothing moved; `moved` and `sum_width` equal the reference exactly."""
import ctypes as C
import os

import numpy as np
import pytest

import arm_layouts
from conftest import ROOT, load_golden
from test_param_deltas import (ERR_ARG, ERR_UNSUPPORTED, ERR_VALUE, INT32_MAX, INT32_MIN, TERM_TOL, _check, _layout, _oracle_total, _ParamCase,
                               _shape_ok, _words)
from test_rate_deltas import _cool_chics

ENTRY_POINTS = ["ccd_enc_measure_ifce_deltas", "ccd_enc_slot_ifce_count", "ccd_enc_slot_ifce_deltas"]
WHOLE = ["ifce0_15_18x65_s6_i3_h3", "ifce3_15_18x65_s9_i7_h6", "ifce1_1_18x65_s6_i3_h3", "ifce4_4_18x65_s9_i7_h6", "tiny3x13_s5_i2_h1"]
# Three of those five cannot meet the conditions of test_inventory_conditions_from_the_oracle: in ifce3_15_18x65_s9_i7_h6 no
# candidate of grids 6 and 7 (three pixels each) moves a symbol, in ifce4_4_18x65_s9_i7_h6 every candidate moves one (no row with
# moved == 0), in tiny3x13_s5_i2_h1 grids 2 .. 8 (four pixels to one) answer to nothing - and so it is in every tiny case of
# arm_layouts at every seed 0 .. 199.  The conditions are asserted on the same shapes and placements at another seed
# (arm_layouts.make_case: (kind, shape, ifce_resolution, size, seed, extreme latents?)), the one-hidden-layer shape at 18 x 65 with
# IFCE on grids 0 .. 3; the five cases named above keep their whole-table runs beside them.
RESEEDED = {"ifce3_15_18x65_s9_i7_h6@7400": ("placement", (9, 7, 6), (3, 15), (18, 65), 7400, False),
            "ifce4_4_18x65_s9_i7_h6@7201": ("placement", (9, 7, 6), (4, 4), (18, 65), 7201, True),
            "ifce0_3_18x65_s5_i2_h1@7300": ("placement", (5, 2, 1), (0, 3), (18, 65), 7300, False)}
INVENTORY = [WHOLE[0], WHOLE[2]] + list(RESEEDED)
ZERO_HIDDEN = "arm_s39_i31_h0"
SAMPLED = ["vid3_hop/1/0", "vid3_hop/1/1", ZERO_HIDDEN]
REFINED = WHOLE[0]


# ---- the cases -------------------------------------------------------------------------------------------------------
class _IfceCase(_ParamCase):
    """test_param_deltas._ParamCase counted from the first IFCE integer: reference(k, sign) is values[n_arm + k] + sign."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.n_ifce = self.layout[2] + self.layout[3]
        self.n_if = int(self.arch.output_feature_ifce)
        self.fin = [int(self.arch.input_features_ifce[g]) for g in range(self.arch.n_grids)]

    def reference(self, k, sign):
        assert 0 <= k < self.n_ifce
        return super().reference(self.n_arm + k, sign)

    def place(self, k):
        """(grid, feature, source channel or -1 for a bias) of IFCE integer k: the stream's order restated (the weights
        [n_ifce_out][fin_g] of every grid with IFCE in grid order, then those grids' biases)."""
        n_w = self.layout[2]
        r = k - n_w if k >= n_w else k
        for g, fin in enumerate(self.fin):
            block = 0 if fin == 0 else (self.n_if if k >= n_w else self.n_if * fin)
            if r < block:
                return (g, r, -1) if k >= n_w else (g, r // fin, r % fin)
            r -= block
        raise IndexError(k)

    def grid_blocks(self):
        """{grid: (first weight, last weight, first bias, last bias)} in IFCE integer numbering."""
        out, w, b = {}, 0, self.layout[2]
        for g, fin in enumerate(self.fin):
            if fin:
                out[g] = (w, w + self.n_if * fin - 1, b, b + self.n_if - 1)
                w += self.n_if * fin
                b += self.n_if
        return out

    def all_pairs(self):
        return [(k, s) for k in range(self.n_ifce) for s in (-1, 1)]


_CASES = {}


def _case(oracle, name):
    """A case by name, made once per process with the references it has been asked for."""
    if name not in _CASES:
        if name.startswith("vid3_hop"):
            _, frame, cc = name.split("/")
            _, frames = oracle.split_stream(load_golden("vid3_hop")[0])
            _CASES[name] = _IfceCase(oracle, name, *frames[int(frame)][1][int(cc)])
        else:
            c = arm_layouts.make_case((name,) + RESEEDED[name]) if name in RESEEDED else _layout(name)
            _CASES[name] = _IfceCase(oracle, name, c.hdr, c.nn, c.payload)
    return _CASES[name]


def _sample(case):
    """At most 64 candidates: both ends of every grid's weight block and bias block with both signs, the rest seeded with one
    seeded sign each."""
    must = list(dict.fromkeys(k for ends in case.grid_blocks().values() for k in ends))
    pairs = [(k, s) for k in must for s in (-1, 1)]
    assert len(pairs) <= 64
    rng = np.random.default_rng(2121)
    rest = [k for k in range(case.n_ifce) if k not in set(must)]
    n_more = min(64 - len(pairs), len(rest))
    pairs += [(rest[i], int(rng.choice((-1, 1)))) for i in rng.choice(len(rest), size=n_more, replace=False)] if n_more else []
    return pairs


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
    assert all(hasattr(EncodeBatch, m) for m in ("measure_ifce_deltas", "ifce_deltas", "ifce_count"))
    assert cool_chic_amd.RateRefiner is nnrefine.RateRefiner and issubclass(nnrefine.RateRefiner, nnrefine.ArmRefiner)
    for name in ("rate_expgol_bit_deltas", "rate_payload_byte_deltas"):
        assert callable(getattr(nnrefine, name))
    first, count = C.c_int(7), C.c_int(7)
    assert L.ccd_enc_measure_ifce_deltas(None, None, 0, -1, 0) == ERR_ARG
    assert L.ccd_enc_slot_ifce_count(None, 0) == ERR_ARG
    assert L.ccd_enc_slot_ifce_deltas(None, 0, C.byref(first), C.byref(count), None, None, None) == ERR_ARG
    assert (first.value, count.value) == (7, 7)


@pytest.mark.parametrize("name", ["vid3_hop/0/0"] + WHOLE + [ZERO_HIDDEN])
def test_plan_through_python(oracle, name):
    from cool_chic_amd import writer
    from cool_chic_amd._lib import CCHeader
    from cool_chic_amd.nnrefine import (build_candidate, expgol_bit_deltas, payload_byte_deltas, rate_expgol_bit_deltas,
                                        rate_payload_byte_deltas)

    if name.startswith("vid3_hop"):
        hdr, nn, _ = _cool_chics(oracle, load_golden("vid3_hop")[0])[0]
    else:
        c = _layout(name)
        hdr, nn = c.hdr, c.nn
    arch = writer.parse_cc_header(hdr)
    values = writer.network_values(arch, nn)
    layout = writer.network_layout(arch)
    n_arm, n_ifce = sum(layout[:2]), sum(layout[2:4])
    assert n_ifce > 0

    def payload(v):
        h = CCHeader.from_buffer_copy(bytes(arch))
        out = writer.encode_network(h, v)
        return 8 * len(out) - h.nn_n_bit_pad, writer.network_values(h, out)

    base, back = payload(values)
    assert base == 8 * len(nn) - arch.nn_n_bit_pad and np.array_equal(back, values)
    table = rate_expgol_bit_deltas(arch, values)
    rechosen = rate_payload_byte_deltas(arch, values)
    assert table.shape == rechosen.shape == (n_arm + n_ifce, 2) and table.dtype == rechosen.dtype == np.float64
    # the ARM's rows are the existing tables', bit for bit
    assert table[:n_arm].view(np.uint64).tolist() == expgol_bit_deltas(arch, values).view(np.uint64).tolist()
    assert rechosen[:n_arm].view(np.uint64).tolist() == payload_byte_deltas(arch, values).view(np.uint64).tolist()
    _, nn0 = build_candidate(arch, values)
    for k in range(n_ifce):
        for j, s in enumerate((-1, 1)):
            v = values.copy()
            v[n_arm + k] += s
            bits, got = payload(v)
            assert np.flatnonzero(got != values).tolist() == [n_arm + k] and got[n_arm + k] == values[n_arm + k] + s, (k, s)
            assert table[n_arm + k, j] == bits - base, (k, s)
            if name == "ifce1_1_18x65_s6_i3_h3":  # the refiner's own table: bytes with every order chosen again
                assert rechosen[n_arm + k, j] == 8 * (len(build_candidate(arch, v)[1]) - len(nn0)), (k, s)
    # the int32 edges: a move that cannot be transmitted
    v = values.copy()
    v[n_arm], v[n_arm + n_ifce - 1] = INT32_MAX, INT32_MIN
    for t in (rate_expgol_bit_deltas(arch, v), rate_payload_byte_deltas(arch, v)):
        assert t[n_arm, 1] == np.inf and t[-1, 0] == np.inf and np.isfinite(t[n_arm, 0]) and np.isfinite(t[-1, 1])
        assert np.isinf(t).sum() == 2
    with pytest.raises(ValueError):
        rate_expgol_bit_deltas(arch, values[:-1])


class _World:
    """A made-up rate for RateRefiner's hooks: bits(values) = 10 000 + sum weight[k] * |values[k] - target[k]| (100 a unit), additive over the
    integers, so an honest table's promises add up and 100 bits outweigh any change of the payload (a code moves by at most two
    bits, the payload by at most a byte)."""

    def __init__(self, arch, values, n_arm, n_rate, targets):
        self.arch, self.n_arm, self.n_rate = arch, n_arm, n_rate
        self.target = np.asarray(values, np.int64).copy()
        for k, d in targets.items():
            self.target[k] += d
        self.weight = np.full(self.target.size, 100.0)  # bits per unit of distance
        self.lies = {}       # (k, column) -> the promise put in place of the truth
        self.n_tables = self.n_prices = 0

    def bits(self, values):
        return 10000.0 + float((self.weight * np.abs(np.asarray(values, np.int64) - self.target)).sum())

    def values_of(self, h, nn):
        from cool_chic_amd import writer

        return writer.network_values(h, nn)

    def table(self, h, nn, ptrs, owner, stream):
        from cool_chic_amd.encoder import ParamDeltas

        self.n_tables += 1
        v = np.asarray(self.values_of(h, nn), np.int64)[:self.n_rate]
        t = self.target[:self.n_rate]
        bits = np.stack([self.weight[:self.n_rate] * (np.abs(v + s - t) - np.abs(v - t)) for s in (-1, 1)], axis=1).astype(np.float64)
        for (k, j), promise in self.lies.items():
            bits[k, j] = promise
        moved = (bits != 0).astype(np.int64)
        return self.bits(self.values_of(h, nn)), ParamDeltas(0, bits, np.zeros_like(moved), moved)

    def price(self, h, nn, ptrs, owner, stream):
        self.n_prices += 1
        return self.bits(self.values_of(h, nn))


def _fake_refiner(monkeypatch, world, modules):
    from cool_chic_amd.nnrefine import RateRefiner

    r = RateRefiner(0, modules=modules)
    monkeypatch.setattr(r, "_table", world.table)
    monkeypatch.setattr(r, "_price", world.price)
    return r


def test_refiner_with_a_fake_table(monkeypatch):
    from cool_chic_amd import writer
    from cool_chic_amd.nnrefine import RateRefiner

    c = _layout("ifce1_1_18x65_s6_i3_h3")
    arch, values = c.arch, writer.network_values(c.arch, c.nn)
    layout = writer.network_layout(arch)
    n_arm, n_rate = sum(layout[:2]), sum(layout[:4])
    arm_k, ifce_k = [3, 40, 200], [n_arm + 1, n_arm + 9, n_arm + 20, n_rate - 1]
    targets = {k: (2 if i % 2 else -2) for i, k in enumerate(arm_k + ifce_k)}

    def descends(res):
        objective = res.start_objective
        for step in res.log:
            assert step.objective < objective and step.objective == step.total_bits + 8.0 * step.n_bytes_nn
            assert all(true >= objective for _, _, true in step.rejected)
            objective = step.objective
        return [m.index for step in res.log for m in step.moves]

    # IFCE alone, honest table: every move is an IFCE index, the batch is taken whole, it ends when no move promises a gain
    world = _World(arch, values, n_arm, n_rate, targets)
    res = _fake_refiner(monkeypatch, world, ("ifce",)).refine(arch, values, [], max_steps=10, batch=3)
    touched = descends(res)
    assert touched and all(n_arm <= k < n_rate for k in touched) and set(touched) == set(ifce_k)
    # four integers two units from their target: eight unit moves, at most one per integer and three per step, none rejected
    sizes = [len(s.moves) for s in res.log]
    assert res.stopped == "no move promises a gain" and sum(sizes) == 8 and sizes[:2] == [3, 3] and max(sizes) == 3 and not any(s.rejected for s in res.log)
    assert np.array_equal(res.values[:n_arm], values[:n_arm])
    assert np.array_equal(res.values[ifce_k], world.target[ifce_k])
    # both modules: one pick over both ranges; max_steps ends it
    world = _World(arch, values, n_arm, n_rate, targets)
    res = _fake_refiner(monkeypatch, world, ("arm", "ifce")).refine(arch, values, [], max_steps=2, batch=4)
    touched = descends(res)
    assert res.stopped == "max_steps" and len(res.log) == 2 and any(k < n_arm for k in touched) and any(k >= n_arm for k in touched)
    assert set(touched) <= set(arm_k + ifce_k)
    # ("arm",) is ArmRefiner's choice of rows
    world = _World(arch, values, n_arm, n_rate, targets)
    res = _fake_refiner(monkeypatch, world, ("arm",)).refine(arch, values, [], max_steps=10, batch=8)
    assert set(descends(res)) == set(arm_k) and res.stopped == "no move promises a gain"
    # a table that overshoots: one good IFCE move and seven promised gains that are losses - 8, 4, 2 are rejected, 1 is accepted
    world = _World(arch, values, n_arm, n_rate, {ifce_k[0]: -1})
    for i in range(7):
        world.lies[(n_arm + 10 + i, 1)] = -90.0 + i
        world.weight[n_arm + 10 + i] = 300.0  # one such loss outweighs the good move, so the pair is rejected as well
    res = _fake_refiner(monkeypatch, world, ("arm", "ifce")).refine(arch, values, [], max_steps=1, batch=8)
    step, = res.log
    assert [n for n, _, _ in step.rejected] == [8, 4, 2] and [(m.index, m.sign) for m in step.moves] == [(ifce_k[0], -1)]
    assert descends(res) == [ifce_k[0]]
    # the same lies in the ARM's rows are not looked at when the IFCE alone is refined
    world = _World(arch, values, n_arm, n_rate, {ifce_k[0]: -1})
    for i in range(7):
        world.lies[(5 + i, 1)] = -900.0
    res = _fake_refiner(monkeypatch, world, ("ifce",)).refine(arch, values, [], max_steps=3, batch=8)
    assert descends(res) == [ifce_k[0]] and not res.log[0].rejected and res.stopped == "no move promises a gain"
    # every promise a lie: the best single move does not lower the objective, nothing is accepted, the network is the one given
    world = _World(arch, values, n_arm, n_rate, {})
    world.lies[(n_arm + 2, 0)] = -50.0
    res = _fake_refiner(monkeypatch, world, ("ifce",)).refine(arch, values, [], max_steps=5, batch=4)
    assert res.stopped == "the best single move does not lower the objective" and not res.log and np.array_equal(res.values, values)
    assert world.n_tables == 1 and world.n_prices == 1
    for bad in ((), ("ifce", "ifce"), ("synthesis",)):
        with pytest.raises(ValueError):
            RateRefiner(0, modules=bad)


def test_case_inventory(oracle):
    """The GPU cases hold what they are there for."""
    cases = {name: _case(oracle, name) for name in WHOLE + list(RESEEDED) + SAMPLED}
    for name in RESEEDED:  # the reseeded cases are the named ones in architecture
        twin = cases[name.split("@")[0]] if name.split("@")[0] in cases else None
        assert twin is None or (twin.fin, twin.n_if, twin.dim, twin.n_layers) == (cases[name].fin, cases[name].n_if, cases[name].dim, cases[name].n_layers)
    assert cases["ifce0_3_18x65_s5_i2_h1@7300"].n_layers == 2 and cases["ifce0_3_18x65_s5_i2_h1@7300"].fin == [9, 8, 7, 6] + [0] * 6
    whole = [cases[n] for n in WHOLE]
    assert any(f >= 2 for c in whole for f in c.fin)                                   # a grid with fin >= 2
    assert all(c.fin[-1] == 1 for c in (cases[WHOLE[0]], cases[WHOLE[1]], cases[WHOLE[4]]))  # IFCE on the last grid
    hyper = cases["ifce4_4_18x65_s9_i7_h6"]
    hw = [(hyper.arch.grid_h[g], hyper.arch.grid_w[g]) for g in range(hyper.arch.n_grids)]
    assert hyper.arch.flag_hyperlatent and hyper.fin[4] > 0 and hyper.fin[5] > 0 and hw[4] == hw[5]  # a latent grid and the hyperlatent grid of its level
    gap = cases["ifce3_15_18x65_s9_i7_h6"]
    assert any(gap.fin[g] == 0 and gap.fin[g + 1] > 0 for g in range(len(gap.fin) - 1))   # a grid without IFCE above one with
    assert cases["ifce1_1_18x65_s6_i3_h3"].fin == [0, 8] + [0] * 8                        # ... and below
    assert gap.n_if == 7 and hyper.n_if == 7                                               # n_ifce_out odd
    first = cases[WHOLE[0]]
    assert any(first.fin[g] > 0 and first.arch.grid_w[g] <= 9 and first.arch.grid_h[g] > 1 for g in range(first.arch.n_grids))  # raster
    assert first.n_ifce == 168 and gap.n_ifce == 203 and cases[WHOLE[4]].n_ifce == 112
    # 0, 1, 2 and >= 3 hidden layers: no layer behind the features, the output layer behind layer 0, scratch columns from 2 on
    hidden = {c.n_layers - 1 for c in cases.values()}
    assert {0, 1, 2, 3, 6} <= hidden
    assert cases[ZERO_HIDDEN].n_layers == 1 and cases[WHOLE[4]].n_layers == 2 and cases["vid3_hop/1/0"].n_layers == 3
    assert cases["vid3_hop/1/0"].n_ifce == 108 and cases["vid3_hop/1/1"].n_ifce == 10 and cases["vid3_hop/1/1"].arch.n_grids == 5
    for name in SAMPLED:
        pairs = _sample(cases[name])
        assert len(pairs) <= 64 and len(set(pairs)) == len(pairs)
        ends = {k for e in cases[name].grid_blocks().values() for k in e}
        assert all((k, s) in pairs for k in ends for s in (-1, 1))
    # more than one 64-pixel block and more than one chunk of 32 blocks in a grid with IFCE
    big = cases["vid3_hop/1/0"]
    assert big.arch.grid_h[0] * big.arch.grid_w[0] > 32 * 64 and big.fin[0] > 0
    assert first.arch.grid_h[0] * first.arch.grid_w[0] % 64 != 0


@pytest.mark.parametrize("name", INVENTORY)
def test_inventory_conditions_from_the_oracle(oracle, name):
    """Conditions on the references, not measurements of the device: every grid with sources answers to a weight and to a
    bias, something moves nothing, and the coarsest grid's weights (an all-zero channel) move nothing at all."""
    case = _case(oracle, name)
    refs = {(k, s): case.reference(k, s) for k, s in case.all_pairs()}
    n_grids = case.arch.n_grids
    for g, fin in enumerate(case.fin):
        if not arm_layouts.has_sources(case.arch, g):
            continue
        for bias in (False, True):
            assert any(m > 0 for (k, s), (_, _, m) in refs.items() if case.place(k)[0] == g and (case.place(k)[2] < 0) == bias), (name, g, bias)
    assert any(m == 0 for _, _, m in refs.values()), name
    for (k, s), (bits, width, moved) in refs.items():
        g, _, c = case.place(k)
        if g == n_grids - 1 and c >= 0:
            assert (bits, width, moved) == (0.0, 0, 0), (name, k, s)
        assert moved <= case.arch.grid_h[g] * case.arch.grid_w[g]  # only symbols of its own grid can answer


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
        assert enc.ifce_count(0) == case.n_ifce
        enc.measure_ifce_deltas(first=first, count=count, mode=mode)
        enc.wait()
        return enc.ifce_deltas(0)
    finally:
        enc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", WHOLE + list(RESEEDED))
def test_whole_table_against_the_oracle(gpu, oracle, name):
    case = _case(oracle, name)
    table = _table(gpu, case)
    _shape_ok(table, 0, case.n_ifce)
    assert np.isfinite(table.bits).all()
    worst = _check(case, table, case.all_pairs(), "whole table")
    for k in range(case.n_ifce):  # the coarsest grid's weights: exactly 0.0, 0, 0
        g, _, c = case.place(k)
        if g == case.arch.n_grids - 1 and c >= 0:
            assert table.bits[k].view(np.uint64).tolist() == [0, 0] and not table.moved[k].any() and not table.sum_width[k].any()
    still = int((table.moved == 0).sum())
    print(f"{name}: {2 * case.n_ifce} candidates, {case.n_decodes} oracle decodes, {still} move nothing, "
          f"worst deviation {worst:.3g} of the bound")


@pytest.mark.gpu
@pytest.mark.parametrize("name", SAMPLED)
def test_sampled_table_against_the_oracle(gpu, oracle, name):
    case = _case(oracle, name)
    pairs = _sample(case)
    table = _table(gpu, case)
    _shape_ok(table, 0, case.n_ifce)
    worst = _check(case, table, pairs, "sampled table")
    assert case.n_decodes <= 64, case.n_decodes
    print(f"{name}: dim {case.dim}, {case.n_layers} layers, {case.n_ifce} IFCE integers on grids {sorted(case.grid_blocks())}, {len(pairs)} "
          f"candidates, worst deviation {worst:.3g} of the bound")


@pytest.mark.gpu
def test_modes(gpu, oracle):
    """mode 1 (generic), mode 2 (incremental) and mode 0 give the same words on every case, whole table.  arm_s40_i31_h7's state
    (8 x 71 columns per lane) does not fit the LDS: mode 2 is CCD_ERR_UNSUPPORTED before any device work, the handle stays
    usable and mode 0 gives mode 1's words there."""
    from cool_chic_amd._lib import CcdError, lib

    n_moved = 0
    for name in WHOLE + list(RESEEDED) + SAMPLED:
        case = _case(oracle, name)
        enc = gpu(0)
        enc.add(case.arch, case.nn, case.latents)
        words = {}
        for mode in (1, 2, 0):
            enc.measure_ifce_deltas(mode=mode); enc.wait()
            t = enc.ifce_deltas(0)
            _shape_ok(t, 0, case.n_ifce)
            words[mode] = _words(t)
            n_moved += int((t.moved > 0).sum()) if mode == 2 else 0
        enc.close()
        assert words[2] == words[1], name
        assert words[0] == words[1], name
    assert n_moved > 500  # the comparison is not one of empty tables
    wide = _layout("arm_s40_i31_h7")
    case = _IfceCase(oracle, wide.name, wide.hdr, wide.nn, wide.payload)
    enc = gpu(0)
    enc.add(case.arch, case.nn, case.latents)
    enc.measure_ifce_deltas(count=16, mode=1); enc.wait()
    generic, rate = _words(enc.ifce_deltas(0)), enc.rate(0)
    with pytest.raises(CcdError) as e:
        enc.measure_ifce_deltas(count=16, mode=2)
    assert e.value.code == ERR_UNSUPPORTED
    # refused before the device was touched: nothing is in flight, the last table and the meter's results stand
    assert lib().ccd_enc_wait(enc._h, None) == 0
    assert _words(enc.ifce_deltas(0)) == generic and enc.rate(0).total_bits == rate.total_bits
    enc.measure_ifce_deltas(count=16, mode=0); enc.wait()
    assert _words(enc.ifce_deltas(0)) == generic
    for kwargs in (dict(mode=3), dict(mode=-1), dict(first=-1)):
        with pytest.raises(CcdError) as e:
            enc.measure_ifce_deltas(**kwargs)
        assert e.value.code == ERR_ARG
    assert _words(enc.ifce_deltas(0)) == generic  # refusals leave the table alone
    enc.close()


@pytest.mark.gpu
def test_a_slot_gives_the_same_words_alone_in_a_batch_twice_and_by_range(gpu, oracle):
    case = _case(oracle, "ifce3_15_18x65_s9_i7_h6")
    alone = gpu(0)
    alone.add(case.arch, case.nn, case.latents)
    alone.measure_ifce_deltas(); alone.wait()
    full = alone.ifce_deltas(0)
    want = _words(full)
    alone.measure_ifce_deltas(); alone.wait()  # a second call
    assert _words(alone.ifce_deltas(0)) == want
    n = case.n_ifce
    for first, count in ((0, 1), (3, 64), (37, 65), (100, 80), (n - 1, 1), (n - 1, 5), (60, -1), (150, 10)):  # sub-ranges: rows of the full table
        alone.measure_ifce_deltas(first=first, count=count); alone.wait()
        t = alone.ifce_deltas(0)
        rows = min(count if count >= 0 else n, n - first)
        _shape_ok(t, first, rows)
        assert t.bits.view(np.uint64).tolist() == full.bits[first:first + rows].view(np.uint64).tolist(), (first, count)
        assert np.array_equal(t.sum_width, full.sum_width[first:first + rows]) and np.array_equal(t.moved, full.moved[first:first + rows])
    alone.measure_ifce_deltas(first=500, count=4); alone.wait()  # a range past the slot's parameters: clipped to nothing
    _shape_ok(alone.ifce_deltas(0), n, 0)
    alone.close()
    # as slot 2 behind two slots of other architectures, one of them without IFCE
    none, other = _layout("tiny5x34_s6_i0_h2"), _case(oracle, "tiny3x13_s5_i2_h1")
    bare = _IfceCase(oracle, none.name, none.hdr, none.nn, none.payload)
    assert bare.n_ifce == 0
    mixed = gpu(0)
    mixed.add(bare.arch, bare.nn, bare.latents)
    mixed.add(other.arch, other.nn, other.latents)
    assert mixed.add(case.arch, case.nn, case.latents) == 2
    mixed.measure(); mixed.wait()
    plain = mixed.rate(0)
    mixed.measure_ifce_deltas(); mixed.wait()
    assert _words(mixed.ifce_deltas(2)) == want
    assert mixed.ifce_count(0) == 0 and mixed.ifce_count(1) == other.n_ifce
    _shape_ok(mixed.ifce_deltas(0), 0, 0)  # no IFCE: an empty table, and the meter's results as after measure()
    r = mixed.rate(0)
    assert r.status == 0 and np.concatenate([r.bits, [r.total_bits]]).view(np.uint64).tolist() == np.concatenate([plain.bits, [plain.total_bits]]).view(np.uint64).tolist()
    _check(other, mixed.ifce_deltas(1), [(0, -1), (other.n_ifce - 1, 1)], "in a batch")
    mixed.measure_ifce_deltas(mode=2); mixed.wait()  # a slot without IFCE refuses no mode
    assert _words(mixed.ifce_deltas(2)) == want
    mixed.close()


@pytest.mark.gpu
def test_meter_and_arm_table_are_untouched(gpu, oracle):
    from cool_chic_amd._lib import CcdError

    case = _case(oracle, "ifce1_1_18x65_s6_i3_h3")
    enc = gpu(0)
    enc.add(case.arch, case.nn, case.latents)
    enc.measure(); enc.wait()
    plain = enc.rate(0)
    enc.measure_param_deltas(); enc.wait()
    arm = _words(enc.param_deltas(0))
    with pytest.raises(CcdError) as e:  # the handle's table is the ARM's
        enc.ifce_deltas(0)
    assert e.value.code == ERR_ARG
    enc.measure_ifce_deltas(); enc.wait()
    r = enc.rate(0)
    assert r.status == plain.status == 0
    assert np.concatenate([r.bits, [r.total_bits]]).view(np.uint64).tolist() == np.concatenate([plain.bits, [plain.total_bits]]).view(np.uint64).tolist()
    assert r.sum_width.tolist() == plain.sum_width.tolist() and r.n_symbols.tolist() == plain.n_symbols.tolist()
    assert (r.n_bytes_nn, r.n_bytes_header) == (plain.n_bytes_nn, plain.n_bytes_header)
    want = _words(enc.ifce_deltas(0))
    for call in (lambda: enc.param_deltas(0), lambda: enc.delta_map(0, 0), lambda: enc.rate_map(0, 0)):
        with pytest.raises(CcdError) as e:
            call()
        assert e.value.code == ERR_ARG
    enc.run(); enc.wait()  # a run leaves the table alone
    assert _words(enc.ifce_deltas(0)) == want
    enc.measure_param_deltas(); enc.wait()  # the ARM's table afterwards: the words it gave before
    assert _words(enc.param_deltas(0)) == arm
    with pytest.raises(CcdError) as e:
        enc.ifce_deltas(0)
    assert e.value.code == ERR_ARG
    enc.measure_ifce_deltas(); enc.wait()
    assert _words(enc.ifce_deltas(0)) == want
    enc.measure(); enc.wait()  # the next measure of any kind invalidates it
    for call in (lambda: enc.ifce_deltas(0), lambda: enc.param_deltas(0)):
        with pytest.raises(CcdError) as e:
            call()
        assert e.value.code == ERR_ARG
    enc.close()


@pytest.mark.gpu
def test_int32_edges(gpu, oracle):
    base = _case(oracle, "tiny3x13_s5_i2_h1")
    c = _layout(base.name)
    values = base.values.copy()
    blocks = base.grid_blocks()
    k_w, k_b = blocks[0][0] + 3, blocks[1][2]  # a weight of grid 0, the first bias of grid 1
    values[base.n_arm + k_w], values[base.n_arm + k_b] = INT32_MAX, INT32_MIN
    case = _IfceCase(oracle, base.name + " at the int32 edges", c.hdr, c.nn, c.payload, values=values)
    table = _table(gpu, case)
    _shape_ok(table, 0, case.n_ifce)
    for k, j in ((k_w, 1), (k_b, 0)):
        assert table.bits[k, j] == np.inf and table.sum_width[k, j] == 0 and table.moved[k, j] == 0
    assert np.isinf(table.bits).sum() == 2
    pairs = [(k_w, -1), (k_b, 1)] + [(k, s) for k in (k_w - 1, k_w + 1, k_b - 1, k_b + 1, 0, case.n_ifce - 1) for s in (-1, 1)]
    worst = _check(case, table, pairs, "int32 edges")
    print(f"int32 edges: {len(pairs)} pairs, worst deviation {worst:.3g} of the bound")


@pytest.mark.gpu
def test_poisoned_device_latent_is_that_slots_error_only(gpu, oracle):
    import torch

    from cool_chic_amd._lib import CcdError

    case = _case(oracle, "ifce1_1_18x65_s6_i3_h3")
    planes = [[torch.as_tensor(a, device="cuda").contiguous() for a in case.latents] for _ in range(3)]
    planes[1][1][3, 5] = 64
    torch.cuda.synchronize()
    enc = gpu(0)
    for s in range(3):
        enc.add_device(case.arch, case.nn, [p.data_ptr() for p in planes[s]], owner=planes[s])
    enc.measure_ifce_deltas()
    with pytest.raises(CcdError) as e:
        enc.wait()
    assert e.value.code == ERR_VALUE
    assert enc.rate(1).status == ERR_VALUE
    with pytest.raises(CcdError) as e:
        enc.ifce_deltas(1)
    assert e.value.code == ERR_VALUE
    for s in (0, 2):
        assert enc.rate(s).status == 0
        _check(case, enc.ifce_deltas(s), case.all_pairs(), "beside a poisoned slot")
    enc.close()


# ---- the refiner -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_latents(gpu, oracle):
    import torch

    case = _case(oracle, REFINED)
    planes = [torch.as_tensor(a, device="cuda").contiguous() for a in case.latents]
    torch.cuda.synchronize()
    return case, [p.data_ptr() for p in planes], planes


@pytest.mark.gpu
def test_refiner_single_ifce_moves(device_latents):
    from cool_chic_amd import RateRefiner
    from cool_chic_amd.nnrefine import build_candidate

    case, ptrs, owner = device_latents
    res = RateRefiner(0, modules=("ifce",)).refine(case.arch, case.values, ptrs, max_steps=6, batch=1, owner=owner)
    assert res.log and len(res.log) <= 6
    # the best single IFCE move by exhaustive enumeration on the CPU, orders chosen again for every candidate (the refiner's rule)
    base_total = case.total_bits()
    _, nn0 = build_candidate(case.arch, case.values)
    best = None
    for k, s in case.all_pairs():
        v = case.values.copy()
        v[case.n_arm + k] += s
        d_bits, _, moved = case.reference(k, s)
        key = (base_total + d_bits + 8.0 * len(build_candidate(case.arch, v)[1]), case.n_arm + k, s, moved)
        if best is None or key < best:
            best = key
    first = res.log[0]
    print(f"start {res.start_objective!r} (CPU {base_total + 8.0 * len(nn0)!r}); best single IFCE move on the CPU: integer {best[1]} at "
          f"{best[2]:+d}, {best[0]!r}; the refiner's first step: {[(m.index, m.sign) for m in first.moves]}, {first.objective!r}")
    assert abs(first.objective - best[0]) <= 2.0 * best[3] * TERM_TOL, (first.objective, best)
    assert [(m.index, m.sign) for m in first.moves] == [(best[1], best[2])] and not first.rejected
    objective, values = res.start_objective, case.values.copy()
    for i, step in enumerate(res.log):  # strictly decreasing, IFCE indices only
        assert step.objective < objective, (i, step.objective, objective)
        assert len(step.moves) == 1 and case.n_arm <= step.moves[0].index < case.n_arm + case.n_ifce
        values[step.moves[0].index] += step.moves[0].sign
        objective = step.objective
    assert np.array_equal(values, res.values) and np.array_equal(res.values[:case.n_arm], case.values[:case.n_arm])
    # the returned stream: the same latents in the oracle, and the oracle's bits are the last logged ones (the meter's bound)
    lat, total = _oracle_total(case, res.header, res.bytes_nn)
    assert all(np.array_equal(a, b) for a, b in zip(lat, case.latents))
    assert abs(total - res.log[-1].total_bits) <= case.n_symbols * TERM_TOL, (total, res.log[-1].total_bits)
    print(f"{len(res.log)} steps ({res.stopped}): {res.start_objective:.2f} -> {res.log[-1].objective:.2f} bits, "
          f"network {len(nn0)} -> {len(res.bytes_nn)} bytes")


@pytest.mark.gpu
def test_refiner_both_modules_against_the_arm_alone(device_latents):
    from cool_chic_amd import ArmRefiner, RateRefiner

    case, ptrs, owner = device_latents
    arm = ArmRefiner(0).refine(case.arch, case.values, ptrs, max_steps=5, batch=1, owner=owner)
    both = RateRefiner(0).refine(case.arch, case.values, ptrs, max_steps=5, batch=1, owner=owner)
    assert both.start_objective == arm.start_objective and both.log
    end_arm = arm.log[-1].objective if arm.log else arm.start_objective
    assert both.log[-1].objective <= end_arm, (both.log[-1].objective, end_arm)
    touched = [m.index for step in both.log for m in step.moves]
    from_arm, from_ifce = [k for k in touched if k < case.n_arm], [k for k in touched if k >= case.n_arm]
    assert all(k < case.n_arm + case.n_ifce for k in touched)
    if not (from_arm and from_ifce):
        print("no gain in the", "IFCE's" if from_arm else "ARM's", "table within 5 steps")
    print(f"ARM alone: {arm.start_objective:.2f} -> {end_arm:.2f}; ARM + IFCE: -> {both.log[-1].objective:.2f}, integers {touched}")
