"""Joint RDOQ steps of two slots on one claim raster (ccd_rdoq_link, RdoqStep.link, InterRdEvaluator.descend(joint=True); DESIGN.md
sections 4.14 "Groups" and 4.15): the candidates of a linked pair compete in one key order, so a step's moves are pairwise
independent across both cool-chics of a P / B frame and the frame's squared error changes by the sum of both slots' chosen entries.

CPU: the entry point and its argument errors; the numpy restatement of the rounds over a pair (tests/rdoq_joint_ref.py) against
itself - at its fixed point the walk in key order, pairwise independent across both slots, maximal - and the conditions that keep
the seeded and crafted cases honest.
GPU, synthetic and crafted maps: every result of both slots equals the restatement exactly, n_open per slot included; a slot whose
mask is 0 makes the link inert, a plain slot beside a pair steps as without it, a step leaves a clean state, a refused link
leaves the handle as it was.
GPU, end to end on vid3_ldp frame 1: a joint step's moves are the restatement's, the evaluated SSE moves by the sum of both
d_sse as integers, each cool-chic's bits by its d_bits within the rate deltas' bound; the joint descent ends; the alternating
descent is what it was; tools/requantise_video.py --joint writes a stream that decodes to what it scored."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import rdoq_joint_ref as jr
from conftest import GOLDEN, ROOT
from test_rdoq import ERR_ARG, ERR_VALUE, _compare, _device_outcome, _fresh, _reference_step, _Synth, _words, gpu  # noqa: F401  (gpu: the fixture)

ROUNDS = [1, 2, 3, 64]


# ---- crafted offers (costs kD = kR = 1: the cost of an offer is its dD) ----------------------------------------------------------------
def _coarse(geo):
    """The coarsest latent grid whose latent (0, 0) has the whole raster as its box."""
    whole = (0, 0, geo.cells_h - 1, geo.cells_w - 1)
    return max(g for g in range(geo.n) if not geo.hyper[g] and tuple(geo.boxes()[g][0, 0]) == whole)


def _tie():
    """Equal costs at the same position of both slots: the boxes are equal, the leader's candidate has the smaller key."""
    case = jr.CraftedPair("odd18x65")
    for slot in (0, 1):
        case.offer(slot, 0, 30, 9, -100)
    return case, {1: ([[(0, 0, 30, 9)]], (0, 1)), 2: ([[(0, 0, 30, 9)], []], (0, 0))}


def _uid_boundary():
    """Equal costs at the leader's last latent (uid total - 1) and the follower's first (uid total).  Their boxes do not meet, so both
    are selected in round 1; a follower candidate that meets the first and a leader candidate that meets the second lose, and are
    blocked in round 2 only if the cells of both winners were settled as taken: the lookup of the owner at both sides of the boundary."""
    case = jr.CraftedPair("odd18x65")
    geo = case.geo
    last = geo.n - 1
    hl, wl = geo.hw[last]
    h, w = geo.hw[0]
    case.offer(0, last, hl - 1, wl - 1, -100)
    case.offer(1, 0, 0, 0, -100)
    case.offer(1, 0, h - 1, w - 1, -50)  # meets the leader's last latent
    case.offer(0, 0, 0, 0, -50)          # meets the follower's first latent
    boxes = geo.boxes()
    assert jr._rects_meet(boxes[last][hl - 1, wl - 1], boxes[0][h - 1, w - 1]) and not jr._rects_meet(boxes[last][hl - 1, wl - 1], boxes[0][0, 0])
    cands = case.cands()
    keys = sorted(c[0] & 0xFFFFFFFF for c in cands if c[0] >> 32 == min(k[0] for k in cands) >> 32)
    assert keys == [case.pair.offset[1] - 1, case.pair.offset[1]]  # the two winners' uids are neighbours
    return case, {1: ([[(0, last, hl - 1, wl - 1), (1, 0, 0, 0)]], (1, 1)), 2: ([[(0, last, hl - 1, wl - 1), (1, 0, 0, 0)], []], (0, 0))}


def _big(cost):
    """A follower candidate whose box is the whole raster (384 cells: a wave walks them) against leader candidates a lane walks:
    at -200 it loses the corner to the leader's -300 and holds every other cell in round 1; at -400 it holds them all."""
    case = jr.CraftedPair("rgb192")
    geo = case.geo
    coarse = _coarse(geo)
    assert geo.cells_h * geo.cells_w > 32
    lanes = [(0, 0, 0), (0, 127, 191), (0, 64, 96), (0, 10, 100)]
    case.offer(1, coarse, 0, 0, cost)
    case.offer(0, *lanes[0], -300)
    for p in lanes[1:]:
        case.offer(0, *p, -100)
    if cost == -200:
        return case, {1: ([[(0,) + lanes[0]]], (3, 1)), 2: ([[(0,) + lanes[0]], [(0,) + p for p in sorted(lanes[1:])]], (0, 0))}
    return case, {1: ([[(1, coarse, 0, 0)]], (4, 0)), 2: ([[(1, coarse, 0, 0)], []], (0, 0))}


def _relay(name, mirrored):
    """L loses round 1 to F, whose box is the whole raster and which loses the far corner to X: round 1 selects X, round 2 blocks F and
    selects L.  L and X are the leader's and F the follower's, or (mirrored) the other way round."""
    case = jr.CraftedPair(name)
    geo = case.geo
    h, w = geo.hw[0]
    a, b = int(mirrored), 1 - int(mirrored)
    case.offer(a, 0, 0, 0, -300)                # X
    case.offer(b, _coarse(geo), 0, 0, -200)     # F
    case.offer(a, 0, h - 1, w - 1, -100)        # L
    assert not jr._rects_meet(geo.boxes()[0][0, 0], geo.boxes()[0][h - 1, w - 1])
    opens = (1, 1)
    return case, {1: ([[(a, 0, 0, 0)]], opens), 2: ([[(a, 0, 0, 0)], [(a, 0, h - 1, w - 1)]], (0, 0))}


CRAFTED = {"tie": _tie, "uid boundary": _uid_boundary, "big loses a corner": lambda: _big(-200), "big wins": lambda: _big(-400),
           "relay": lambda: _relay("odd18x65", False), "relay mirrored": lambda: _relay("odd18x65", True),
           "relay, a wave's box": lambda: _relay("rgb192", False), "relay mirrored, a wave's box": lambda: _relay("rgb192", True)}


def _where(per_round):
    return [sorted(c[1:5] for c in won) for won in per_round]


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def link():
    """The entry point the restatement describes: without it there is nothing to restate."""
    from cool_chic_amd import _lib

    assert "ccd_rdoq_link" in _lib.SIGNATURES
    return _lib.lib().ccd_rdoq_link


def test_link_is_declared_exported_bound_and_checks_its_arguments_first():
    from cool_chic_amd import RdoqStep, _lib, rd_inter

    with open(os.path.join(ROOT, "include", "ccd.h")) as f:
        header = f.read()
    L = _lib.lib()
    assert "ccd_rdoq_link(" in header and "ccd_rdoq_link" in _lib.SIGNATURES and L.ccd_rdoq_link is not None
    assert hasattr(RdoqStep, "link")
    assert rd_inter.InterJointStepReport._fields == ("before", "steps") and rd_inter.InterStepReport._fields == ("before", "role", "step")
    handle = C.create_string_buffer(512)  # stands for a handle: the calls must return before they look at it
    r = C.cast(handle, C.c_void_p)
    assert L.ccd_rdoq_link(None, 1, 0) == ERR_ARG
    for slot, leader in ((-1, 0), (0, -1), (-1, -1), (0, 0), (3, 3)):
        assert L.ccd_rdoq_link(r, slot, leader) == ERR_ARG, (slot, leader)
    assert bytes(handle) == bytes(512)


@pytest.mark.parametrize("label", list(jr.PAIRS))
def test_the_pair_rounds_end_at_the_greedy_walk_and_the_cases_are_honest(link, label):
    pair, syns, own, cands = jr.seeded(label)
    per_round, n_certified = jr.fixed_point(pair, cands)
    selected = [c for won in per_round for c in won]
    assert sorted(selected) == jr.greedy(pair, cands)
    # pairwise independent across both slots: no cell lies in two selected boxes; maximal: every other candidate meets a selected box
    count = np.zeros((pair.cells_h, pair.cells_w), np.int64)
    for c in selected:
        count[pair.box(c)] += 1
    assert count.max(initial=0) <= 1
    keys = {c[0] for c in selected}
    assert len(keys) == len(selected) and len({c[0] for c in cands}) == len(cands)  # the group-wide keys are distinct
    assert all(count[pair.box(c)].any() for c in cands if c[0] not in keys)
    assert n_certified in (len(per_round), len(per_round) + 1)
    # every truncation is a prefix of the rounds, and nothing is open from the certified round on
    for r in range(1, n_certified + 2):
        got = jr.Rounds(pair, cands, r)
        assert got.per_round[:len(per_round)] == per_round[:r] and (got.n_open == (0, 0)) == (r >= n_certified)
    # the follower's keys are its own slot's keys plus the leader's latents; the candidates are each slot's own
    assert [c[0] - pair.offset[c[1]] for c in cands] == [c[0] for k in range(2) for c in own[k]]
    full = jr.Rounds(pair, cands, 64)
    n_sel = [sum(1 for c in selected if c[1] == k) for k in range(2)]
    print(f"{label}: {[len(o) for o in own]} candidates, moves per round {[len(w) for w in per_round]}, per slot {n_sel}, nothing open after "
          f"{n_certified} rounds, lost to {sorted(full.lost_to)}, blocked by {sorted(full.blocked_by)}")
    # the conditions that keep the case honest: moves of each slot, cells lost across the slots both ways, a leader candidate blocked
    # in a later round by a cell a selected FOLLOWER candidate owns (the settle lookup), three rounds or more
    assert min(n_sel) >= 1
    assert {(0, 1), (1, 0)} <= full.lost_to
    assert (0, 1) in full.blocked_by
    assert len(per_round) >= 3


@pytest.mark.parametrize("what", list(CRAFTED))
def test_crafted_offers_in_the_restatement(link, what):
    case, expect = CRAFTED[what]()
    pair, cands = case.pair, case.cands()
    for rounds, (winners, n_open) in expect.items():
        got = jr.Rounds(pair, cands, rounds)
        assert _where(got.per_round) == [sorted(w) for w in winners] and got.n_open == n_open, (what, rounds, _where(got.per_round), got.n_open)
    per_round, _ = jr.fixed_point(pair, cands)
    assert sorted(c for won in per_round for c in won) == jr.greedy(pair, cands)


# ---- GPU: synthetic and crafted maps -----------------------------------------------------------------------------------------------
def _step_of(gpu, syns, links, kD, kR, masks, rounds):
    """A fresh handle with the slots of `syns`, the links [(slot, leader)], one step.  Returns (handle, outcome per slot)."""
    step = gpu(0)
    for s in syns:
        s.add_to(step)
    for slot, leader in links:
        step.link(slot, leader)
    n = len(syns)
    step.step([kD] * n, [kR] * n, [0.0] * n, masks, rounds=rounds)
    step.wait()
    return step, [_device_outcome(step, k, s) for k, s in enumerate(syns)]


def _check_pair(pair, own, cands, syns, outcomes, rounds, kD, kR, what, host=None, order=(0, 1)):
    """outcomes[order[k]] is the device's slot of the pair's slot k (0 leader, 1 follower).  host: per slot (lat, dd, db), the seeded ones
    by default."""
    want = jr.Rounds(pair, cands, rounds)
    for k in range(2):
        s, outcome = syns[order[k]], outcomes[order[k]]
        lat, dd, db = (s.lat, s.dd, s.db) if host is None else host[k]
        _compare(s, outcome, jr.slot_ref(pair, k, lat, own[k], want.per_round), kD, kR, f"{what}, slot {k}, {rounds} rounds", dd, db)
        assert outcome[0].n_open == want.n_open[k], (what, k, rounds, outcome[0].n_open, want.n_open)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("rounds", ROUNDS)
@pytest.mark.parametrize("label", list(jr.PAIRS))
def test_pairs_against_the_restatement(gpu, label, rounds):
    pair, host, own, cands = jr.seeded(label)
    syns = jr.fresh(label)
    full = [(1 << s.geo.n) - 1 for s in syns]
    step, outcomes = _step_of(gpu, syns, [(1, 0)], host[0].kD, host[0].kR, full, rounds)
    want = _check_pair(pair, own, cands, syns, outcomes, rounds, host[0].kD, host[0].kR, label)
    print(f"{label}, {rounds} rounds: moves {[o[0].n_moves for o in outcomes]}, open {want.n_open}")
    step.close()
    if rounds == 3:  # the follower before the leader in the handle: the same step with the slots exchanged
        syns = jr.fresh(label)[::-1]
        step, outcomes = _step_of(gpu, syns, [(0, 1)], host[0].kD, host[0].kR, full[::-1], rounds)
        _check_pair(pair, own, cands, syns, outcomes, rounds, host[0].kD, host[0].kR, label + ", follower first", order=(1, 0))
        step.close()


@pytest.mark.gpu
def test_every_truncation_of_one_pair(gpu):
    label = "odd18x65"
    pair, host, own, cands = jr.seeded(label)
    per_round, n_certified = jr.fixed_point(pair, cands)
    for rounds in range(1, n_certified + 2):
        syns = jr.fresh(label)
        step, outcomes = _step_of(gpu, syns, [(1, 0)], host[0].kD, host[0].kR, [(1 << s.geo.n) - 1 for s in syns], rounds)
        want = _check_pair(pair, own, cands, syns, outcomes, rounds, host[0].kD, host[0].kR, label)
        assert sum(o[0].n_moves for o in outcomes) == sum(len(w) for w in per_round[:rounds])
        assert (want.n_open == (0, 0)) == (rounds >= n_certified)
        step.close()


@pytest.mark.gpu
@pytest.mark.parametrize("what", list(CRAFTED))
def test_crafted_offers(gpu, what):
    case, expect = CRAFTED[what]()
    pair, own, cands = case.pair, case.own(), case.cands()
    host = [(c.lat, c.dd, c.db) for c in case.cases]
    full = (1 << case.geo.n) - 1
    for rounds in (1, 2, 64):
        syns = case.upload()
        for s, c in zip(syns, case.cases):
            s.lat = c.lat  # (_compare takes the grids' places in the buffer from here)
        step, outcomes = _step_of(gpu, syns, [(1, 0)], 1.0, 1.0, [full, full], rounds)
        want = _check_pair(pair, own, cands, syns, outcomes, rounds, 1.0, 1.0, what, host)
        if rounds in expect:
            assert _where(want.per_round) == [sorted(w) for w in expect[rounds][0]] and want.n_open == expect[rounds][1]
        step.close()


def _all_words(outcomes, step):
    return [(_words(o), step.result(k).n_open) for k, o in enumerate(outcomes)]


@pytest.mark.gpu
@pytest.mark.parametrize("label", ["odd18x65", "yuv420_8b"])
def test_a_slot_without_candidates_makes_the_link_inert(gpu, label):
    _, host, _, _ = jr.seeded(label)
    kD, kR = host[0].kD, host[0].kR
    full = [(1 << s.geo.n) - 1 for s in host]
    for frozen in (1, 0):  # the follower's mask 0, then the leader's
        masks = [0 if k == frozen else m for k, m in enumerate(full)]
        step, outcomes = _step_of(gpu, jr.fresh(label), [(1, 0)], kD, kR, masks, 3)
        linked = _all_words(outcomes, step)
        step.close()
        step, outcomes = _step_of(gpu, jr.fresh(label), [], kD, kR, masks, 3)
        assert _all_words(outcomes, step) == linked, (label, frozen)
        assert outcomes[frozen][0].n_candidates == 0 and outcomes[1 - frozen][0].n_moves >= 2
        step.close()


@pytest.mark.gpu
def test_plain_slots_beside_a_pair(gpu):
    """odd18x65 leader, rgb192, odd18x65 follower, yuv420_8b in one handle, three rounds: the pair is the restatement's, the plain
    slots give the words of a handle that holds them alone."""
    pair, host, own, cands = jr.seeded("odd18x65")
    kD, kR = host[0].kD, host[0].kR
    lead, foll = jr.fresh("odd18x65")
    plain = _fresh(["rgb192", "yuv420_8b"])
    syns = [lead, plain[0], foll, plain[1]]
    step, outcomes = _step_of(gpu, syns, [(2, 0)], kD, kR, [(1 << s.geo.n) - 1 for s in syns], 3)
    _check_pair(pair, own, cands, syns, outcomes, 3, kD, kR, "beside plain slots", order=(0, 2))
    beside = _all_words(outcomes, step)
    step.close()
    for slot, name in ((1, "rgb192"), (3, "yuv420_8b")):
        alone, = _fresh([name])
        step, outcomes = _step_of(gpu, [alone], [], kD, kR, [(1 << alone.geo.n) - 1], 3)
        assert _all_words(outcomes, step)[0] == beside[slot], name
        assert outcomes[0][0].n_moves >= 2
        step.close()


@pytest.mark.gpu
@pytest.mark.parametrize("label", ["odd18x65", "yuv420_8b"])
def test_a_linked_step_leaves_a_clean_state(gpu, label):
    import torch

    pair, host, own, cands = jr.seeded(label)
    kD, kR = host[0].kD, host[0].kR
    syns = jr.fresh(label)
    full = [(1 << s.geo.n) - 1 for s in syns]
    step, outcomes = _step_of(gpu, syns, [(1, 0)], kD, kR, full, 3)
    first = _all_words(outcomes, step)
    for rounds in (3, 1, 3):  # the same handle from the latents as they were: three rounds, a single round after it, three again
        for s in syns:
            s.buf.copy_(torch.from_numpy(s.host_buffer().view(np.int8)))
        torch.cuda.synchronize()
        step.step([kD] * 2, [kR] * 2, [0.0] * 2, full, rounds=rounds)
        step.wait()
        outcomes = [_device_outcome(step, k, s) for k, s in enumerate(syns)]
        if rounds == 3:
            assert _all_words(outcomes, step) == first
        else:
            _check_pair(pair, own, cands, syns, outcomes, 1, kD, kR, label + ", after a step of three rounds")
    step.close()
    step, outcomes = _step_of(gpu, jr.fresh(label), [(1, 0)], kD, kR, full, 3)  # another handle
    assert _all_words(outcomes, step) == first
    step.close()


@pytest.mark.gpu
def test_link_errors_on_a_live_handle(gpu):
    """Slots: odd18x65 twice, rgb192 (another size), odd18x65 added as yuv444 (another frame_data_type).  Every refused link leaves
    the handle as it was: the step after them gives the words of a handle where only link(1, 0) was called."""
    import torch

    from cool_chic_amd._lib import lib

    L = lib()
    pair, host, _, _ = jr.seeded("odd18x65")
    kD, kR = host[0].kD, host[0].kR

    def slots():
        syns = jr.fresh("odd18x65") + _fresh(["rgb192"]) + [_Synth("odd18x65", 2).upload()]
        step = gpu(0)
        for k, s in enumerate(syns):
            if k < 3:
                s.add_to(step)
            else:
                slot = step.add(s.geo.arch, 2, [s.buf.data_ptr() + p for p in s.pos], owner=s.buf)
                step.set_maps(slot, [t.data_ptr() for t in s.dd_dev], [t.data_ptr() for t in s.db_dev], owner=(s.dd_dev, s.db_dev))
        return step, syns

    def run(step, syns):
        step.step([kD] * 4, [kR] * 4, [0.0] * 4, [(1 << s.geo.n) - 1 for s in syns], rounds=3)

    step, syns = slots()
    step.link(1, 0)
    run(step, syns)
    step.wait()
    want = _all_words([_device_outcome(step, k, s) for k, s in enumerate(syns)], step)
    step.close()

    step, syns = slots()
    h = step._h
    assert L.ccd_rdoq_link(h, 2, 0) == ERR_VALUE and L.ccd_rdoq_link(h, 0, 2) == ERR_VALUE  # img_size
    assert L.ccd_rdoq_link(h, 3, 0) == ERR_VALUE and L.ccd_rdoq_link(h, 1, 3) == ERR_VALUE  # frame_data_type
    for slot, leader in ((4, 0), (0, 4), (1, 1000)):                                         # an index past the slots
        assert L.ccd_rdoq_link(h, slot, leader) == ERR_ARG, (slot, leader)
    assert L.ccd_rdoq_link(h, 1, 0) == 0
    assert L.ccd_rdoq_link(h, 1, 0) == ERR_ARG                                               # twice
    assert L.ccd_rdoq_link(h, 2, 1) == ERR_ARG and L.ccd_rdoq_link(h, 3, 1) == ERR_ARG      # a follower cannot lead
    assert L.ccd_rdoq_link(h, 2, 0) == ERR_ARG and L.ccd_rdoq_link(h, 0, 2) == ERR_ARG      # pairs only
    assert L.ccd_rdoq_link(h, 1, 2) == ERR_ARG                                               # a follower cannot follow another
    run(step, syns)
    assert L.ccd_rdoq_link(h, 3, 2) == ERR_ARG                                               # a step in flight
    step.wait()
    assert L.ccd_rdoq_link(h, 3, 2) == ERR_VALUE
    assert _all_words([_device_outcome(step, k, s) for k, s in enumerate(syns)], step) == want
    for s in syns:  # ... and once more after the refusal in flight, from the latents as they were
        s.buf.copy_(torch.from_numpy(s.host_buffer().view(np.int8)))
    torch.cuda.synchronize()
    run(step, syns)
    step.wait()
    assert _all_words([_device_outcome(step, k, s) for k, s in enumerate(syns)], step) == want
    with pytest.raises(Exception):
        step.link(1, 0)
    step.close()


# ---- GPU: end to end on vid3_ldp frame 1 -----------------------------------------------------------------------------------------------
LMBDA, GRIDS = 1e-3, (0, 1, 2)


def _evaluator(case, dev):
    import inter_cases as ic
    from cool_chic_amd import InterRdEvaluator
    from test_inter_deltas import _frame_data

    ev = InterRdEvaluator(0)
    ev.add(case.frame_type, *[(case.cc[r].arch, case.cc[r].nn, case.cc[r].ptrs(dev[r])) for r in ic.ROLES], case.refs, case.gflow, case.taps,
           _frame_data(case.src, case.bd, case.fdt), owner=dev)
    return ev


def _grids(cc, row):
    host = row.cpu().numpy()
    return [host[int(cc.off[g]):int(cc.off[g]) + n].reshape(cc.hw[g]).copy() for g, n in enumerate(cc.sizes)]


@pytest.mark.gpu
def test_one_joint_step_is_the_restatement_and_predicts_exactly(gpu):
    """vid3_ldp frame 1 against the second set's reconstruction, lambda 1e-3, grids (0, 1, 2) of both cool-chics, one step of eight
    rounds: the moves of every grid of both roles are those the restatement selects from the maps the step read, the frame's SSE
    moves by the sum of both d_sse, each cool-chic's bits by its d_bits within the rate deltas' bound, the cost falls, both roles
    move."""
    import torch

    import inter_cases as ic
    from cool_chic_amd.rd import move_scales
    from test_inter_deltas import _frame_data, _step_bound

    case = ic.case("vid3_ldp", 1)
    dev = {r: case.cc[r].lat_dev.clone() for r in ic.ROLES}
    start = [_grids(case.cc[r], dev[r]) for r in ic.ROLES]
    ev = _evaluator(case, dev)
    (rep,), = ev.descend(LMBDA, max_steps=1, grids=GRIDS, rounds=8, joint=True)
    before, steps = rep.before, rep.steps
    # the restatement over the maps the step read
    geos = [jr.geo("vid3_ldp_residue"), jr.geo("vid3_ldp_motion")]
    pair = jr.Pair(*geos)
    kD, kR = move_scales(sum(int(p.numel()) for p in case.src), case.bd, _frame_data(case.src, case.bd, case.fdt).n_pixels, LMBDA)
    own, maps = [], []
    for i, role in enumerate(ic.ROLES):
        assert bytes(geos[i].arch) == bytes(case.cc[role].arch)
        dd = [torch.as_tensor(ev.distortion_delta_map(0, role, g), device="cuda").cpu().numpy() for g in range(geos[i].n)]
        db = [torch.as_tensor(ev.rate_delta_map(0, role, g), device="cuda").cpu().numpy() for g in range(geos[i].n)]
        maps.append((dd, db))
        own.append(_reference_step(geos[i], start[i], dd, db, kD, kR, 0.0, sum(1 << g for g in GRIDS)).cands)
    want = jr.Rounds(pair, pair.cands(own), 8)
    for i, role in enumerate(ic.ROLES):
        ref = jr.slot_ref(pair, i, start[i], own[i], want.per_round)
        now = _grids(case.cc[role], dev[role])
        for g in range(geos[i].n):
            got = torch.as_tensor(ev.step_moves(0, role, g), device="cuda").cpu().numpy()
            assert np.array_equal(got, ref.moves[g]), (role, g, int((got != ref.moves[g]).sum()))
            assert np.array_equal(now[g], ref.after[g]), (role, g)
        assert (steps[i].n_candidates, steps[i].n_moves, steps[i].n_open) == (len(own[i]), len(ref.chosen), want.n_open[i]), (role, steps[i])
        dd, _ = maps[i]
        assert steps[i].d_sse == sum(int(dd[g][(s + 1) // 2, y, x]) for g, y, x, s in ref.chosen)
    print(f"vid3_ldp[1] joint, restatement: {[len(o) for o in own]} candidates, moves per round "
          f"{[[sum(1 for c in w if c[1] == k) for k in range(2)] for w in want.per_round]}, open {want.n_open}")
    # what the step predicts against the next evaluation
    bounds = [_step_bound(ev, 0, role, case.cc[role].arch, int(before.rates[i].n_symbols.sum())) for i, role in enumerate(ic.ROLES)]
    after, = ev.evaluate(LMBDA)
    d_sse = sum(after.quality.sse) - sum(before.quality.sse)
    d_bits = [after.rates[i].total_bits - before.rates[i].total_bits for i in range(2)]
    print(f"vid3_ldp[1] joint: moves {[s.n_moves for s in steps]}, d_sse {d_sse} (steps {[s.d_sse for s in steps]}), d_bits {d_bits!r} "
          f"(steps {[s.d_bits for s in steps]!r}, bounds {[b for b, _ in bounds]}), cost {before.cost!r} -> {after.cost!r}")
    assert d_sse == steps[0].d_sse + steps[1].d_sse
    for i in range(2):
        assert bounds[i][1] == steps[i].n_moves
        assert abs(d_bits[i] - steps[i].d_bits) <= bounds[i][0], (i, d_bits[i], steps[i].d_bits, bounds[i][0])
    assert steps[0].d_cost + steps[1].d_cost < 0 and after.cost < before.cost
    assert steps[0].n_moves >= 1 and steps[1].n_moves >= 1
    with pytest.raises(ValueError):
        ev.descend(LMBDA, max_steps=1, roles=("residue",), joint=True)
    ev.close()


@pytest.mark.gpu
def test_the_joint_descent_ends_and_every_step_predicts_the_sse(gpu):
    """The joint descent of vid3_ldp frame 1, lambda 1e-3, grids (0, 1, 2), eight rounds, with a least gain of 5e-6: it ends with an
    idle step and every step's predicted SSE is met as integers.  (Without a least gain the descent of this fixture is 629 steps of
    20 106 moves and takes 10 s; 5e-6 - a fifth of the gain of the first step's average move - keeps the moves worth most: 45
    steps, 81 moves of the residue and 52 of the motion cool-chic, under a second.)"""
    import inter_cases as ic

    case = ic.case("vid3_ldp", 1)
    dev = {r: case.cc[r].lat_dev.clone() for r in ic.ROLES}
    ev = _evaluator(case, dev)
    reports = ev.descend(LMBDA, max_steps=200, min_gain=5e-6, grids=GRIDS, rounds=8, joint=True)
    last, = ev.evaluate(LMBDA)
    moves = [[s.n_moves for s in rep[0].steps] for rep in reports]
    print(f"vid3_ldp[1] joint descent: {len(reports)} steps, moves per step {moves}, cost {reports[0][0].before.cost!r} -> {last.cost!r}")
    assert sum(moves[-1]) == 0 and all(sum(m) for m in moves[:-1]), moves  # it ran until a step moved nothing
    assert all(sum(m[k] for m in moves) >= 2 for k in range(2))            # ... and both roles took part
    sse = [sum(rep[0].before.quality.sse) for rep in reports] + [sum(last.quality.sse)]
    for k, rep in enumerate(reports):
        assert sse[k + 1] - sse[k] == rep[0].steps[0].d_sse + rep[0].steps[1].d_sse, k
    assert last.cost < reports[0][0].before.cost
    assert len(ev.descend(LMBDA, max_steps=5, min_gain=5e-6, grids=GRIDS, rounds=8, joint=True)) == 1  # at the fixed point: one idle step
    ev.close()


def _plain(reports):
    return [(rep[0].role, rep[0].step, rep[0].before.cost, rep[0].before.bits, tuple(rep[0].before.quality.sse),
             rep[0].before.rates[0].total_bits, rep[0].before.rates[1].total_bits) for rep in reports]


@pytest.mark.gpu
def test_the_alternating_descent_is_what_it_was(gpu):
    """joint=False on an evaluator whose slots a joint step has linked, from the same latents as an evaluator that never linked:
    the same reports, the same latents."""
    import torch

    import inter_cases as ic

    case = ic.case("vid3_ldp", 1)
    out = []
    for linked in (False, True):
        dev = {r: case.cc[r].lat_dev.clone() for r in ic.ROLES}
        ev = _evaluator(case, dev)
        if linked:
            ev.descend(LMBDA, max_steps=1, grids=GRIDS, rounds=8, joint=True)
            for r in ic.ROLES:
                dev[r].copy_(case.cc[r].lat_dev)
            torch.cuda.synchronize()
        reports = ev.descend(LMBDA, max_steps=4, grids=GRIDS, rounds=4)
        out.append((_plain(reports), [dev[r].cpu().numpy().tobytes() for r in ic.ROLES]))
        assert [rep[0].role for rep in reports] == ["residue", "motion", "residue", "motion"] and reports[0][0].step.n_moves >= 1
        ev.close()
    assert out[0] == out[1]


@pytest.mark.gpu
def test_requantise_video_tool_joint(gpu, tmp_path):
    """tools/requantise_video.py --joint --max-steps 2 --grids 0,1,2 on the stream and source of
    tests/test_inter_deltas.py::test_requantise_video_tool: exit status 0 (its decode-back assertion inside), the output parses, and
    its per-frame costs sum to no more than the input's."""
    import torch

    import inter_cases as ic
    from cool_chic_amd import DecodeBatch
    from cool_chic_amd.bitstream.decode import _split_frame, decode_video
    from cool_chic_amd.bitstream.header import VideoHeader

    parsed = ic.parse_video("vid3_ldp")
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
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "requantise_video.py"), src, yuv, out, "--lmbda", str(LMBDA),
                          "--max-steps", "2", "--grids", "0,1,2", "--joint"], cwd=ROOT, capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stderr[-2000:]
    assert "residue + motion" in run.stdout and "after:" in run.stdout

    def costs(path):
        with open(path, "rb") as f:
            rest = VideoHeader().read_header(f.read())
        frames = decode_video(path)
        total = []
        for k in range(3):  # vid3_ldp: coding order = display order
            n0 = len(rest)
            _, ccs, rest = _split_frame(rest)
            assert len(ccs) == (1 if k == 0 else 2)
            planes = frames[str(k)].integer_planes()
            sse = sum(int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum()) for a, b in zip(planes, sources[k]))
            total.append(sse / (sum(a.size for a in planes) * 255.0 * 255.0) + LMBDA * 8.0 * (n0 - len(rest)) / (128 * 224))
        assert rest == b""
        return total

    before, after = costs(src), costs(out)
    print("cost per frame before", before, "after", after)
    assert sum(after) <= sum(before)
