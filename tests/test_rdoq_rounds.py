"""RDOQ step in rounds (ccd_rdoq_step_rounds, RdoqStep.step(rounds=), descend(rounds=)): after a round the
cells of the winners' boxes are taken, the open candidates that meet them are blocked, and the rest compete again.

CPU: the new entry points and their argument errors; the numpy restatement of the rounds against itself - at its fixed point it
is the walk over the candidates in ascending key order, pairwise independent and maximal, and its first round is
tests/test_rdoq.py::_reference_step.
GPU, synthetic and crafted maps: every truncation (the result after R rounds) equals the restatement exactly, n_open included,
and a step leaves the handle as a fresh one.
GPU, end to end: with rounds the evaluated SSE still moves by d_sse as integers and the bits by d_bits within the rate deltas'
bound; a descent with rounds ends, and its result goes through the device writer and the decoder."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_rdoq import (ERR_ARG, SENTINEL, SYNTHETIC, _compare, _device_outcome, _fresh, _geo, _picture, _Ref, _rects_meet, _reference_step,
                       _step_bound, _Synth, _words, gpu)  # noqa: F401  (gpu: the module's fixture)

NEW_ENTRY_POINTS = ["ccd_rdoq_max_rounds", "ccd_rdoq_step_rounds", "ccd_rdoq_slot_open"]
MASKS = {"all": lambda n: (1 << n) - 1, "grids 0-2": lambda n: 7, "grid 0": lambda n: 1}
ONES = np.uint64(2 ** 64 - 1)


# ---- the rounds in numpy ---------------------------------------------------------------------------------------------------
def _box(geo, c):
    t, l, b, r = geo.boxes()[c[1]][c[2], c[3]]
    return slice(t, b + 1), slice(l, r + 1)


def _reference_rounds(geo, cands, max_rounds):
    """cands: [(key, g, y, x, s)] as _reference_step lists them.  Returns (winners per round, n_open): the candidates each of the
    `max_rounds` rounds selected and those that took part in the last round without being selected."""
    taken = np.zeros((geo.cells_h, geo.cells_w), bool)
    open_, per_round = list(cands), []
    for _ in range(max_rounds):
        if not open_:  # nothing left to compete: the remaining rounds select nothing and leave nothing open
            per_round.append([])
            continue
        open_ = [c for c in open_ if not taken[_box(geo, c)].any()]  # 1. blocked for good
        raster = np.full((geo.cells_h, geo.cells_w), ONES, np.uint64)
        for c in open_:                                                # 2. claim
            np.minimum(raster[_box(geo, c)], np.uint64(c[0]), out=raster[_box(geo, c)])
        won = [c for c in open_ if (raster[_box(geo, c)] == np.uint64(c[0])).all()]  # 3. select
        for c in won:                                                  # 4. their cells are taken
            taken[_box(geo, c)] = True
        won_keys = {c[0] for c in won}
        open_ = [c for c in open_ if c[0] not in won_keys]
        per_round.append(won)
    return per_round, len(open_)


def _greedy(geo, cands):
    """The walk over the candidates in ascending key order: a candidate is taken unless its box holds a taken cell."""
    taken = np.zeros((geo.cells_h, geo.cells_w), bool)
    out = []
    for c in sorted(cands):
        if not taken[_box(geo, c)].any():
            taken[_box(geo, c)] = True
            out.append(c)
    return out


def _fixed_point(geo, cands):
    """(winners per round up to and including the last round that selects, rounds until n_open is 0)."""
    per_round, _ = _reference_rounds(geo, cands, 64)
    n_sel = max((k + 1 for k, w in enumerate(per_round) if w), default=0)
    n_certified = next(r for r in range(1, 66) if _reference_rounds(geo, cands, r)[1] == 0)
    return per_round[:n_sel], n_certified


def _as_ref(geo, lat, cands, per_round):
    """The _Ref (tests/test_rdoq.py) of a step that selected `per_round`."""
    moves = [np.zeros(hw, np.int8) for hw in geo.hw]
    after = [a.copy() for a in lat]
    chosen = []
    for won in per_round:
        for _, g, y, x, s in won:
            moves[g][y, x] = s
            after[g][y, x] += s
            chosen.append((g, y, x, s))
    return _Ref(moves, after, len(cands), chosen, len(cands) - len(chosen), cands)


_CANDS = {}


def _synthetic_cands(name, mask_label):
    """The candidates of _Synth(name, 0) under a mask, min_gain 0, and round 1's choice as _reference_step makes it; once."""
    if (name, mask_label) not in _CANDS:
        s = _Synth(name, 0)
        ref = _reference_step(s.geo, s.lat, s.dd, s.db, s.kD, s.kR, 0.0, MASKS[mask_label](s.geo.n))
        _CANDS[name, mask_label] = (s, ref)
    return _CANDS[name, mask_label]


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_and_argument_errors():
    from cool_chic_amd import _lib, rdoq

    with open(os.path.join(ROOT, "include", "ccd.h")) as f:
        header = f.read()
    L = _lib.lib()
    for name in NEW_ENTRY_POINTS:
        assert name + "(" in header, name
        assert name in _lib.SIGNATURES, name
        assert getattr(L, name) is not None
    assert L.ccd_rdoq_max_rounds() == 64 and rdoq.max_rounds() == 64
    assert rdoq.StepResult._fields[-1] == "n_open" and rdoq.StepResult(0, 0, (), 0, 0.0, 0.0).n_open == 0
    handle = C.create_string_buffer(512)  # stands for a handle: the calls must return before they look at it
    r = C.cast(handle, C.c_void_p)
    one, mask = (C.c_double * 1)(1.0), (C.c_uint64 * 1)(1)
    assert L.ccd_rdoq_step_rounds(None, one, one, one, mask, 1, None) == ERR_ARG
    for args in ((None, one, one, mask), (one, None, one, mask), (one, one, None, mask), (one, one, one, None)):
        assert L.ccd_rdoq_step_rounds(r, *args, 1, None) == ERR_ARG
    for rounds in (0, -1, 65):
        assert L.ccd_rdoq_step_rounds(r, one, one, one, mask, rounds, None) == ERR_ARG, rounds
    assert L.ccd_rdoq_slot_open(None, 0) == ERR_ARG and L.ccd_rdoq_slot_open(r, -1) == ERR_ARG
    assert bytes(handle) == bytes(512)


@pytest.mark.parametrize("mask_label", list(MASKS))
@pytest.mark.parametrize("name", SYNTHETIC)
def test_the_rounds_end_at_the_greedy_walk(name, mask_label):
    syn, first = _synthetic_cands(name, mask_label)
    geo, cands = syn.geo, first.cands
    per_round, n_certified = _fixed_point(geo, cands)
    selected = [c for won in per_round for c in won]
    assert sorted(selected) == _greedy(geo, cands)
    # pairwise independent: no cell lies in two selected boxes; maximal: every other candidate meets a selected box
    count = np.zeros((geo.cells_h, geo.cells_w), np.int64)
    for c in selected:
        count[_box(geo, c)] += 1
    assert count.max(initial=0) <= 1
    keys = {c[0] for c in selected}
    assert all(count[_box(geo, c)].any() for c in cands if c[0] not in keys)
    # the first round is the single selection
    assert [(g, y, x, s) for _, g, y, x, s in per_round[0]] == first.chosen
    assert n_certified in (len(per_round), len(per_round) + 1)
    # every truncation is a prefix of the rounds, and n_open is 0 from the certified round on
    for r in range(1, n_certified + 2):
        got, n_open = _reference_rounds(geo, cands, r)
        assert got[:len(per_round)] == per_round[:r] and (n_open == 0) == (r >= n_certified)
    print(f"{name}, {mask_label}: {len(cands)} candidates, moves per round {[len(w) for w in per_round]}, {len(selected)} in all, "
          f"n_open 0 after {n_certified} rounds")
    if mask_label == "all" and name in ("rgb192", "yuv420_8b"):  # the cases stay honest (19 -> 76 and 27 -> 74 when written)
        assert len(per_round) >= 3 and len(selected) >= 2 * len(per_round[0])


# ---- GPU: synthetic maps -------------------------------------------------------------------------------------------------------
def _run(step, kD, kR, min_gain, masks, rounds):
    step.step(kD, kR, min_gain, masks, rounds=rounds)
    step.wait()


def _unchanged_maps(s):
    return all(np.array_equal(s.dd_dev[g].cpu().numpy(), s.dd[g]) and
               np.array_equal(s.db_dev[g].cpu().numpy().view(np.uint32), s.db[g].view(np.uint32)) for g in range(s.geo.n))


@pytest.mark.gpu
@pytest.mark.parametrize("rounds", [1, 2, 3, 64])
def test_four_architectures_in_one_launch(gpu, rounds):
    from cool_chic_amd._lib import lib

    syns = _fresh(SYNTHETIC)
    step = gpu(0)
    for s in syns:
        s.add_to(step)
    full = [(1 << s.geo.n) - 1 for s in syns]
    _run(step, [s.kD for s in syns], [s.kR for s in syns], [0.0] * len(syns), full, rounds)
    outcomes = []
    for slot, s in enumerate(syns):
        _, first = _synthetic_cands(s.geo.name, "all")
        per_round, n_open = _reference_rounds(s.geo, first.cands, rounds)
        ref = _as_ref(s.geo, s.lat, first.cands, per_round)
        outcomes.append(_device_outcome(step, slot, s))
        _compare(s, outcomes[-1], ref, s.kD, s.kR, f"four in one handle, {rounds} rounds")
        assert outcomes[-1][0].n_open == n_open, (s.geo.name, rounds, outcomes[-1][0].n_open, n_open)
        assert _unchanged_maps(s), s.geo.name
        print(f"{s.geo.name}, {rounds} rounds: {len(first.cands)} candidates, {len(ref.chosen)} moves, {n_open} open")
    step.close()
    if rounds == 1:  # the same words as ccd_rdoq_step on a fresh upload
        again = _fresh(SYNTHETIC)
        plain = gpu(0)
        for s in again:
            s.add_to(plain)
        n = len(again)
        arr = lambda v: (C.c_double * n)(*v)  # noqa: E731
        assert lib().ccd_rdoq_step(plain._h, arr([s.kD for s in again]), arr([s.kR for s in again]), arr([0.0] * n), (C.c_uint64 * n)(*full), None) == 0
        plain.wait()
        for slot, s in enumerate(again):
            assert _words(_device_outcome(plain, slot, s)) == _words(outcomes[slot]), s.geo.name
        plain.close()


class _Crafted:
    """Zeros as latents and no move anywhere (the sentinel in both distortion planes, rate deltas 0.0) except where a case puts one."""

    def __init__(self, name):
        self.syn = s = _Synth(name, 1)
        self.geo = s.geo
        self.lat = [np.zeros_like(a) for a in s.lat]
        self.dd = [np.full_like(a, SENTINEL) for a in s.dd]
        self.db = [np.zeros_like(a) for a in s.db]

    def offer(self, g, y, x, cost, k=0):
        self.dd[g][k, y, x] = cost

    def candidates(self, mask=None, dd_null=()):
        dd = [None if g in dd_null else a for g, a in enumerate(self.dd)]
        return _reference_step(self.geo, self.lat, dd, self.db, 1.0, 1.0, 0.0, (1 << self.geo.n) - 1 if mask is None else mask).cands

    def check(self, gpu, rounds, cands, what, mask=None, dd_null=()):
        """One step of `rounds` rounds on a fresh handle against the restatement; returns (winners per round, n_open)."""
        s = _Synth(self.geo.name, 1).upload(self.lat, self.dd, self.db)
        step = gpu(0)
        s.add_to(step, dd_null)
        _run(step, [1.0], [1.0], [0.0], [(1 << self.geo.n) - 1 if mask is None else mask], rounds)
        per_round, n_open = _reference_rounds(self.geo, cands, rounds)
        dd = [None if g in dd_null else a for g, a in enumerate(self.dd)]
        outcome = _device_outcome(step, 0, s)
        s.lat = self.lat  # (_compare takes the grids' places in the buffer from here)
        _compare(s, outcome, _as_ref(self.geo, self.lat, cands, per_round), 1.0, 1.0, f"{what}, {rounds} rounds", dd, self.db)
        assert outcome[0].n_open == n_open, (what, rounds, outcome[0].n_open, n_open)
        step.close()
        return per_round, n_open


def _ramp(name):
    """One row of grid 0 (rgb192) or one column (odd18x65) with dD = -10000 + 10 t along it: every candidate but the first loses to
    the one before it, so a round selects one move."""
    case = _Crafted(name)
    h, w = case.geo.hw[0]
    if name == "rgb192":
        for x in range(w):
            case.offer(0, h // 2, x, -10000 + 10 * x)
    else:
        for y in range(h):
            case.offer(0, y, w // 2, -10000 + 10 * y)
    return case


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rgb192", "odd18x65"])
def test_ramp_every_truncation(gpu, name):
    case = _ramp(name)
    cands = case.candidates()
    per_round, n_certified = _fixed_point(case.geo, cands)
    assert len(cands) == (case.geo.hw[0][1] if name == "rgb192" else case.geo.hw[0][0])
    assert len(per_round) >= 3 and all(len(won) == 1 for won in per_round)  # (13 rounds on rgb192 and 5 on odd18x65 when written)
    print(f"{name}: {len(cands)} candidates, {len(per_round)} rounds of one move, n_open 0 after {n_certified}")
    for rounds in range(1, len(per_round) + 2):
        got, n_open = case.check(gpu, rounds, cands, "ramp")
        assert sum(len(w) for w in got) == min(rounds, len(per_round))
        assert (n_open == 0) == (rounds >= n_certified)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rgb192", "odd18x65"])
def test_a_loser_no_longer_blocks(gpu, name):
    case = _Crafted(name)
    geo = case.geo
    h, w = geo.hw[0]
    whole = (0, 0, geo.cells_h - 1, geo.cells_w - 1)
    coarse = max(g for g in range(geo.n) if not geo.hyper[g] and tuple(geo.boxes()[g][0, 0]) == whole)  # the coarsest latent grid
    a, b = (0, 0, 0), (0, h - 1, w - 1)
    assert not _rects_meet(geo.boxes()[0][0, 0], geo.boxes()[0][h - 1, w - 1])  # far apart
    case.offer(*a, -300)            # A: the best key
    case.offer(coarse, 0, 0, -200)  # C: the whole raster, between the two
    case.offer(*b, -100)            # B: the worst
    cands = case.candidates()
    assert len(cands) == 3
    got, n_open = case.check(gpu, 1, cands, "a loser")
    assert [[c[1:4] for c in won] for won in got] == [[a]] and n_open == 2
    got, n_open = case.check(gpu, 2, cands, "a loser")
    assert [[c[1:4] for c in won] for won in got] == [[a], [b]] and n_open == 0  # C is blocked
    got, n_open = case.check(gpu, 64, cands, "a loser")
    assert sum(len(won) for won in got) == 2 and n_open == 0


@pytest.mark.gpu
def test_extremes_in_64_rounds(gpu):
    name = "odd18x65"
    geo = _geo(name)
    # all costs equal: the position decides, in every round
    case = _Crafted(name)
    case.dd = [np.full_like(a, -7) for a in case.dd]
    cands = case.candidates()
    got, n_open = case.check(gpu, 64, cands, "equal costs")
    chosen = [c for won in got for c in won]
    assert len(cands) == sum(geo.sizes) and all(c[4] == -1 for c in chosen) and chosen[0][1:4] == (0, 0, 0)
    assert sorted(chosen) == _greedy(geo, cands) and len(got[1]) >= 1 and n_open == 0
    # nothing on offer
    case = _Crafted(name)
    got, n_open = case.check(gpu, 64, case.candidates(), "nothing on offer")
    assert not any(got) and n_open == 0
    # a stale map that offers +1 at 63: never moves, in any round
    case = _Crafted(name)
    case.lat = [np.full_like(a, 63) for a in case.lat]
    for g in range(geo.n):
        case.dd[g][1] = -7
    cands = case.candidates()
    got, n_open = case.check(gpu, 64, cands, "stale +1 at 63")
    assert not cands and not any(got) and n_open == 0
    # the seeded maps: a NULL distortion map for grid 0; a single-grid mask
    seeded = _Synth(name, 1)
    case = _Crafted(name)
    case.lat, case.dd, case.db = seeded.lat, seeded.dd, seeded.db
    cands = case.candidates(dd_null=(0,))
    got, n_open = case.check(gpu, 64, cands, "no distortion map for grid 0", dd_null=(0,))
    assert len(cands) > 0 and sorted(c for won in got for c in won) == _greedy(geo, cands) and n_open == 0
    cands = case.candidates(mask=1 << 1)
    got, n_open = case.check(gpu, 64, cands, "grid 1 alone", mask=1 << 1)
    chosen = [c for won in got for c in won]
    assert chosen and all(c[1] == 1 for c in chosen) and n_open == 0


@pytest.mark.gpu
def test_a_step_leaves_a_clean_state(gpu):
    import torch

    full = [(1 << _geo(n).n) - 1 for n in SYNTHETIC]

    def args(syns):
        return [s.kD for s in syns], [s.kR for s in syns], [0.0] * len(syns), full[:len(syns)]

    # three rounds, then new maps and latents, then step(): word for word a fresh handle's step()
    syns, other = _fresh(SYNTHETIC, 0), [_Synth(n, 1) for n in SYNTHETIC]
    step = gpu(0)
    for s in syns:
        s.add_to(step)
    _run(step, *args(syns), 3)
    three = [_words(_device_outcome(step, k, s)) for k, s in enumerate(syns)]
    opens = [step.result(k).n_open for k in range(len(syns))]
    for slot, (s, o) in enumerate(zip(syns, other)):
        s.buf.copy_(torch.from_numpy(o.host_buffer().view(np.int8)))
        s.dd_dev = [torch.from_numpy(a).cuda() for a in o.dd]
        s.db_dev = [torch.from_numpy(a).cuda() for a in o.db]
        step.set_maps(slot, [t.data_ptr() for t in s.dd_dev], [t.data_ptr() for t in s.db_dev], owner=(s.dd_dev, s.db_dev))
    torch.cuda.synchronize()
    _run(step, *args(syns), 1)
    second = [_words(_device_outcome(step, k, s)) for k, s in enumerate(syns)]
    step.close()
    fresh = _fresh(SYNTHETIC, 1)
    plain = gpu(0)
    for s in fresh:
        s.add_to(plain)
    plain.step(*args(fresh))
    plain.wait()
    assert [_words(_device_outcome(plain, k, s)) for k, s in enumerate(fresh)] == second
    assert all(plain.result(k).n_moves >= 1 for k in range(len(fresh)))  # (a slot's smallest key is always selected)
    plain.close()
    # three rounds again on another handle: the same words, the same n_open; and every slot alone
    syns = _fresh(SYNTHETIC, 0)
    step = gpu(0)
    for s in syns:
        s.add_to(step)
    _run(step, *args(syns), 3)
    assert [_words(_device_outcome(step, k, s)) for k, s in enumerate(syns)] == three
    for s in syns:  # ... and on the same handle from the latents as they were
        s.buf.copy_(torch.from_numpy(s.host_buffer().view(np.int8)))
    torch.cuda.synchronize()
    _run(step, *args(syns), 3)
    assert [_words(_device_outcome(step, k, s)) for k, s in enumerate(syns)] == three
    assert [step.result(k).n_open for k in range(len(syns))] == opens
    step.close()
    for k, name in enumerate(SYNTHETIC):
        s, = _fresh([name])
        alone = gpu(0)
        s.add_to(alone)
        _run(alone, [s.kD], [s.kR], [0.0], [full[k]], 3)
        assert _words(_device_outcome(alone, 0, s)) == three[k] and alone.result(0).n_open == opens[k], name
        alone.close()


# ---- GPU: end to end -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rgb192", "yuv420_8b", "odd18x65"])
def test_one_step_of_eight_rounds_predicts_exactly(gpu, oracle, name):
    from cool_chic_amd import RdEvaluator

    pic = _picture(oracle, name)
    lmbda = 1e-3
    steps = {}
    for rounds in (1, 8):
        dev = pic.device_latents()  # the same starting latents
        ev = RdEvaluator(0)
        ev.add(pic.geo.arch, pic.geo.nn, pic.ptrs(dev), pic.source, owner=dev)
        (rep,), = ev.descend(lmbda, max_steps=1, grids=(0, 1, 2), rounds=rounds)
        before, step = rep.before, rep.step
        steps[rounds] = step
        if rounds == 8:
            bound, n = _step_bound(ev, 0, pic, int(before.rate.n_symbols.sum()))
            after, = ev.evaluate(lmbda)
            d_sse = sum(after.quality.sse) - sum(before.quality.sse)
            d_bits = after.rate.total_bits - before.rate.total_bits
            print(f"{name}: {step.n_candidates} candidates, {steps[1].n_moves} moves in one round, {step.n_moves} in eight ({step.n_open} open), "
                  f"d_sse {d_sse} (step {step.d_sse}), d_bits {d_bits!r} (step {step.d_bits!r}, |diff| {abs(d_bits - step.d_bits):.3g}, "
                  f"bound {bound:.3g}), d_cost {steps[1].d_cost!r} -> {step.d_cost!r}")
            assert n == step.n_moves
            assert d_sse == step.d_sse
            assert abs(d_bits - step.d_bits) <= bound
        ev.close()
    assert steps[8].n_candidates == steps[1].n_candidates and steps[1].n_open > 0
    assert steps[8].n_moves >= steps[1].n_moves >= 1 and -steps[8].d_cost >= -steps[1].d_cost > 0


@pytest.mark.gpu
def test_descent_in_rounds_ends_and_round_trips(gpu, oracle):
    from cool_chic_amd import DecodeBatch, EncodeBatch, RdEvaluator, writer

    pic = _picture(oracle, "odd18x65")
    dev = pic.device_latents()
    ev = RdEvaluator(0)
    ev.add(pic.geo.arch, pic.geo.nn, pic.ptrs(dev), pic.source, owner=dev)
    # (the picture is 18 samples wide: a step holds a handful of moves, and the seeded tenth of the latents takes many steps)
    reports = ev.descend(1e-3, max_steps=400, grids=(0, 1, 2), rounds=8)
    moves = [rep[0].step.n_moves for rep in reports]
    print(f"odd18x65, rounds=8: moves per step {moves}, open {[rep[0].step.n_open for rep in reports]}")
    assert moves[0] >= 2 and moves[-1] == 0 and all(moves[:-1]), moves  # it ran until nothing moved
    final, = ev.evaluate(1e-3)
    assert final.cost < reports[0][0].before.cost
    enc, dec = EncodeBatch(0), DecodeBatch(0)
    enc.add_device(pic.geo.arch, pic.geo.nn, pic.ptrs(dev), owner=dev)
    enc.run(); enc.wait()
    cc = enc.bytes(0)
    h2 = writer.parse_cc_header(cc)
    a, b = h2.n_bytes_header, h2.n_bytes_header + h2.nn_n_bytes
    dec.add(cc[:a], cc[a:b], cc[b:], pic.geo.bd, pic.geo.fdt)
    dec.run(); dec.wait()
    for got, want in zip(dec.planes(0), ev._dec.planes(0)):
        assert np.array_equal(got, want)
    for g, want in enumerate(pic.grids(dev)):
        assert np.array_equal(dec.latent(0, g), want), g
    assert any(not np.array_equal(a_, b_) for a_, b_ in zip(pic.grids(dev), pic.moved))
    enc.close(); dec.close(); ev.close()


@pytest.mark.gpu
def test_inter_descent_in_rounds_predicts_the_sse(gpu):
    """vid3_ldp frame 1, grids (0, 1, 2), rounds=4, one step per role: the frame's SSE is before + d_sse exactly."""
    import inter_cases as ic
    from cool_chic_amd import InterRdEvaluator
    from test_inter_deltas import _frame_data

    case = ic.case("vid3_ldp", 1)
    lmbda = 1e-3
    dev = {r: case.cc[r].lat_dev.clone() for r in ic.ROLES}
    ev = InterRdEvaluator(0)
    ev.add(case.frame_type, *[(case.cc[r].arch, case.cc[r].nn, case.cc[r].ptrs(dev[r])) for r in ic.ROLES], case.refs, case.gflow, case.taps,
           _frame_data(case.src, case.bd, case.fdt), owner=dev)
    for role in ic.ROLES:
        mine = dev[role].clone()
        (rep,), = ev.descend(lmbda, max_steps=1, grids=(0, 1, 2), roles=(role,), rounds=4)
        after, = ev.evaluate(lmbda)
        step = rep.step
        print(f"vid3_ldp[1] {role}, rounds=4: {step.n_candidates} candidates, {step.n_moves} moves, {step.n_open} open, d_sse {step.d_sse}")
        assert step.n_moves >= 1 and int((dev[role] != mine).sum()) == step.n_moves
        assert sum(after.quality.sse) - sum(rep.before.quality.sse) == step.d_sse
        assert step.d_cost < 0 and after.cost < rep.before.cost
    ev.close()


@pytest.mark.gpu
def test_requantise_tool_with_rounds(gpu, oracle, tmp_path):
    """tools/requantise.py --rounds 8 on rgb192 against the picture a seeded change of its latents decodes to: exit status 0 (the
    tool asserts that what it wrote decodes to the planes it scored), steps that moved, and an output that parses."""
    from cool_chic_amd import writer
    from cool_chic_amd.bitstream.header import FrameHeader, VideoHeader

    pic = _picture(oracle, "rgb192")
    assert pic.geo.fdt == 0 and pic.geo.bd == 8
    dec = _decode_moved(pic)
    src, out = str(tmp_path / "source.ppm"), str(tmp_path / "out.cool")
    with open(src, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (pic.geo.W, pic.geo.H) + np.stack(dec, axis=-1).astype(np.uint8).tobytes())
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "requantise.py"), os.path.join(GOLDEN, "rgb192.cool"), src, out,
                          "--lmbda", "1e-3", "--max-steps", "2", "--grids", "0,1,2", "--rounds", "8"], cwd=ROOT, capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stderr[-2000:]
    assert "step 0:" in run.stdout and "still open" in run.stdout and "after:" in run.stdout
    with open(out, "rb") as f:
        rest = FrameHeader().read_header(VideoHeader().read_header(f.read()))
    h2 = writer.parse_cc_header(rest)
    assert h2.n_bytes_header + h2.nn_n_bytes + h2.n_bytes_latent == len(rest)


def _decode_moved(pic):
    from cool_chic_amd import DecodeBatch

    dec = DecodeBatch(0)
    dec.add_latents(pic.geo.arch, pic.geo.nn, pic.moved, pic.geo.bd, pic.geo.fdt)
    dec.run(); dec.wait()
    planes = [np.asarray(p).copy() for p in dec.planes(0)]
    dec.close()
    return planes
