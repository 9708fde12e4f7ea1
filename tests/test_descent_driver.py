"""The host loops of the rate-distortion layer, driven without a device: rdoq.run_step (the one step every descent takes),
rdoq.grid_mask, rdoq.check_lambda, the cycle of role sets in InterRdEvaluator.descend, and the one sweep behind nnquant.search_steps
and nnquant_inter.search_steps_pair.

The handle is a fake that records its calls and hands out scripted StepResults; InterRdEvaluator gets that handle, fake map
tables and a fake evaluate().  Slots are tiny (2 frames, 2 grids); the addresses are made-up integers that nothing dereferences."""
import types

import numpy as np
import pytest
import torch

import test_inter_network_quantiser as pair_tests
import test_network_quantiser as intra_tests
from cool_chic_amd._handle import _DevArray, dev_ptr
from cool_chic_amd.rdoq import SlotMaps, StepResult, check_lambda, grid_mask, run_step

N_GRIDS = 2


class FakeRdoq:
    """Records (name, args) of every call.  `moves`: per step the moves every slot with a non-zero mask reports."""

    def __init__(self, n_slots, moves=()):
        self.n_slots, self.script, self.calls, self.masks = n_slots, list(moves), [], None

    def __len__(self):
        return self.n_slots

    def named(self, name):
        return [args for n, args in self.calls if n == name]

    def set_maps(self, slot, dd_ptrs, dbits_ptrs):
        self.calls.append(("set_maps", (slot, dd_ptrs, dbits_ptrs)))

    def set_dep_maps(self, slot, dep_ptrs):
        self.calls.append(("set_dep_maps", (slot, dep_ptrs)))

    def link(self, slot, leader):
        self.calls.append(("link", (slot, leader)))

    def step(self, kD, kR, min_gain, grid_mask, stream=0, rounds=1):
        self.calls.append(("step", (kD, kR, min_gain, grid_mask, stream, rounds)))
        self.masks, self.moved = list(grid_mask), self.script.pop(0) if self.script else 0

    def wait(self, stream=0):
        self.calls.append(("wait", (stream,)))

    def result(self, slot):
        n = self.moved if self.masks[slot] else 0
        return StepResult(n, n, (n, 0), -n, 0.0, -float(n))


# ---- 1. the step function ----------------------------------------------------------------------------------------------------------
def test_run_step_hands_every_slot_its_maps_then_steps_and_waits():
    h = FakeRdoq(3, [5])
    slots = [SlotMaps(0.5, 2.0, 3, [11, 12], [21, 22], [31, 32]),   # own, rate and dependent maps
             SlotMaps(0.25, 4.0, 0, None, [23, 24]),                # a frozen slot: no distortion maps, dependent maps left alone
             SlotMaps(0.125, 8.0, 1, [15, 16], [25, 26], None)]     # dependent maps explicitly none
    results = run_step(h, 77, slots, 0.5, rounds=4)
    assert h.named("set_maps") == [(0, [11, 12], [21, 22]), (1, [None] * N_GRIDS, [23, 24]), (2, [15, 16], [25, 26])]
    assert h.named("set_dep_maps") == [(0, [31, 32]), (2, None)]
    (kD, kR, min_gain, masks, stream, rounds), = h.named("step")
    assert (kD, kR, masks, stream, rounds) == ([0.5, 0.25, 0.125], [2.0, 4.0, 8.0], [3, 0, 1], 77, 4)
    assert min_gain == [0.5, 0.5, 0.5] and all(type(v) is float for v in min_gain)
    names = [n for n, _ in h.calls]
    assert names.index("step") > max(i for i, n in enumerate(names) if n.startswith("set_")) and names[-2:] == ["step", "wait"]
    assert h.named("wait") == [(77,)]
    assert [r.n_moves for r in results] == [5, 0, 5] and all(isinstance(r, StepResult) for r in results)
    # no slots: one empty step, as a handle without slots takes it
    empty = FakeRdoq(0)
    assert run_step(empty, 0, [], 0.0) == [] and [n for n, _ in empty.calls] == ["step", "wait"]


def test_dev_ptr_reads_the_address_of_a_device_view():
    assert dev_ptr(_DevArray(0x1234, (2, 3), "<i8", None)) == 0x1234 and type(dev_ptr(_DevArray(7, (1,), "|i1", None))) is int


# ---- 2. grid_mask -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_grids, grids", [(7, None), (7, (0, 2, 5)), (4, (-1, 0, 3, 4, 9)), (0, None), (0, (0, 1)), (3, ())])
def test_grid_mask_is_the_literal_expression(n_grids, grids):
    assert grid_mask(n_grids, grids) == sum(1 << g for g in (range(n_grids) if grids is None else grids) if 0 <= g < n_grids)


def test_grid_mask_values():
    assert (grid_mask(7), grid_mask(7, (0, 2, 5)), grid_mask(4, (-1, 0, 3, 4, 9)), grid_mask(0), grid_mask(0, (0, 1))) == (127, 37, 9, 0, 0)


# ---- 3. check_lambda ----------------------------------------------------------------------------------------------------------------
def test_check_lambda():
    for bad in (float("nan"), float("inf"), -float("inf"), -1e-9):
        with pytest.raises(ValueError, match="lmbda and min_gain must be finite and not negative"):
            check_lambda(bad, 0.0)
        with pytest.raises(ValueError, match="lmbda and min_gain must be finite and not negative"):
            check_lambda(1e-3, bad)
        with pytest.raises(ValueError, match="^lmbda must be finite and not negative"):
            check_lambda(bad)
    assert check_lambda(0.0) is None and check_lambda(0.0, 0.0) is None and check_lambda(1e-3, 2.5) is None
    assert check_lambda(np.float32(0.5), np.float64(0.0)) is None


# ---- 4. the cycle of InterRdEvaluator.descend -------------------------------------------------------------------------------------
class FakeMaps:
    """delta_map(slot, grid) of an EncodeBatch or a DistortionDeltas: a view at base + 10 * slot + grid."""

    def __init__(self, base):
        self.base = base

    def delta_map(self, slot, grid):
        return _DevArray(self.base + 10 * slot + grid, (2, 1, 1), "<i8", None)


RATE, OWN = 1000, {0: 2000, 1: 3000}


def _inter(monkeypatch, moves, n_frames=2):
    """An InterRdEvaluator of `n_frames` P frames that holds no device handle: (evaluator, its fake RdoqStep, the roles= of every
    evaluate())."""
    from cool_chic_amd import rd_inter
    from cool_chic_amd._lib import CCHeader

    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=0))
    arch = CCHeader()
    arch.n_grids = N_GRIDS
    source = types.SimpleNamespace(bitdepth=8, n_pixels=16)
    frame = rd_inter._Frame(1, (arch, arch), (b"", b""), ([1, 2], [3, 4]), [], [0, 0, 0, 0], 8, source,
                            [torch.zeros(4, 4, dtype=torch.uint8)] * 3, [])
    ev = object.__new__(rd_inter.InterRdEvaluator)
    ev.device, ev._frames, ev._n_linked = 0, [frame] * n_frames, 0
    ev._rdoq, ev._enc, ev._dd = FakeRdoq(2 * n_frames, moves), FakeMaps(RATE), {r: FakeMaps(b) for r, b in OWN.items()}
    evaluated = []

    def evaluate(lmbda, rate_deltas=False, distortion_deltas=False, roles=rd_inter.ROLES):
        assert rate_deltas and distortion_deltas
        evaluated.append(tuple(roles))
        return [f"before {len(evaluated)}.{k}" for k in range(n_frames)]

    ev.evaluate = evaluate
    return ev, ev._rdoq, evaluated


@pytest.mark.parametrize("roles, joint, moves, max_steps, want_steps", [
    (("residue", "motion"), False, [3, 0, 2, 0, 0], 9, 5),   # stops after a full idle cycle, not after the first idle step
    (("residue", "motion"), False, [0, 0], 9, 2),
    (("motion",), False, [0], 9, 1),
    (("residue", "motion"), True, [4, 0], 9, 2),
    (("residue", "motion"), True, [0], 9, 1),
    (("residue", "motion"), False, [3, 0, 2, 0, 0], 3, 3),   # max_steps caps each
    (("residue", "motion"), False, [0, 0], 1, 1),
    (("motion",), False, [1, 1, 1, 0], 2, 2),
    (("residue", "motion"), True, [4, 4, 4, 0], 3, 3),
    (("motion", "residue"), False, [0, 1, 0, 0], 9, 4),
])
def test_the_descent_stops_after_an_idle_cycle(monkeypatch, roles, joint, moves, max_steps, want_steps):
    from cool_chic_amd.rd_inter import InterJointStepReport, InterStepReport

    ev, h, evaluated = _inter(monkeypatch, moves)
    reports = ev.descend(1e-3, max_steps, roles=roles, joint=joint)
    order = [("residue", "motion").index(r) for r in roles]
    assert len(reports) == len(h.named("step")) == len(h.named("wait")) == len(evaluated) == want_steps
    assert evaluated == ([(0, 1)] * want_steps if joint else [(order[i % len(order)],) for i in range(want_steps)])
    for i, step in enumerate(reports):
        assert [r.before for r in step] == [f"before {i + 1}.{k}" for k in range(2)]
        if joint:
            assert all(type(r) is InterJointStepReport and [s.n_moves for s in r.steps] == [moves[i]] * 2 for r in step)
        else:
            assert all(type(r) is InterStepReport and r.role == roles[i % len(roles)] and r.step.n_moves == moves[i] for r in step)


def test_a_frozen_role_has_mask_zero_and_no_distortion_maps(monkeypatch):
    ev, h, _ = _inter(monkeypatch, [1, 1, 0, 0])
    ev.descend(1e-3, 9, min_gain=0.25, grids={"residue": (0,), "motion": (0, 1, 5)}, rounds=3)
    steps, maps = h.named("step"), h.named("set_maps")
    assert len(steps) == 4 and len(maps) == 4 * 4 and h.named("set_dep_maps") == [] and h.named("link") == []
    rate = lambda s: [RATE + 10 * s, RATE + 10 * s + 1]                      # noqa: E731
    own = lambda s: [OWN[s % 2] + 10 * (s // 2), OWN[s % 2] + 10 * (s // 2) + 1]  # noqa: E731
    for i, (kD, kR, min_gain, masks, stream, rounds) in enumerate(steps):
        moving = i % 2
        assert masks == [(1, 3)[s % 2] if s % 2 == moving else 0 for s in range(4)]
        assert maps[4 * i:4 * i + 4] == [(s, own(s) if s % 2 == moving else [None] * N_GRIDS, rate(s)) for s in range(4)]
        assert min_gain == [0.25] * 4 and rounds == 3 and stream == 0
        assert kD == [1.0 / (48 * 255.0 * 255.0)] * 4 and kR == [1e-3 / 16] * 4


def test_a_joint_step_moves_both_roles_and_links_each_frame_once(monkeypatch):
    ev, h, evaluated = _inter(monkeypatch, [2, 0, 0])
    ev.descend(1e-3, 9, grids=(1,), joint=True)
    ev.descend(1e-3, 9, joint=True)
    assert h.named("link") == [(1, 0), (3, 2)] and ev._n_linked == 2 and evaluated == [(0, 1)] * 3
    first = [n for n, _ in h.calls].index("step")
    assert [n for n, _ in h.calls[:first]] == ["link", "link"] + ["set_maps"] * 4  # linked before the first step
    steps, maps = h.named("step"), h.named("set_maps")
    assert [s[3] for s in steps] == [[2] * 4, [2] * 4, [3] * 4]
    assert all(dd == [OWN[s % 2] + 10 * (s // 2) + g for g in range(N_GRIDS)] for s, dd, _ in maps) and len(maps) == 12
    # the links stay: an alternating descent afterwards freezes the other role as before and links nothing again
    h.script = [0, 0]
    ev.descend(1e-3, 9)
    assert len(h.named("link")) == 2 and [s[3] for s in h.named("step")[3:]] == [[3, 0, 3, 0], [0, 3, 0, 3]]


def test_descend_checks_its_arguments_in_order_before_anything_runs(monkeypatch):
    ev, h, evaluated = _inter(monkeypatch, [])
    with pytest.raises(ValueError, match="no role may move"):
        ev.descend(float("nan"), 1, roles=(), joint=True)
    with pytest.raises(ValueError, match="a joint descent moves both roles"):
        ev.descend(float("nan"), 1, roles=("motion",), joint=True)
    with pytest.raises(ValueError, match="lmbda and min_gain must be finite and not negative"):
        ev.descend(1e-3, 1, min_gain=-1.0)
    assert h.calls == [] and evaluated == []


# ---- 5. the sweep -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("has_ifce", [True, False])
def test_one_network_and_the_first_of_a_pair_are_swept_alike(has_ifce):
    """search_steps and search_steps_pair price the same (module, steps) sequence when the pair's second network never moves: it
    has no IFCE and its finest cell always wins."""
    from cool_chic_amd.nnquant import search_steps
    from cool_chic_amd.nnquant_inter import search_steps_pair

    tables, finest = intra_tests.TABLES, pair_tests.FINEST
    rng = np.random.default_rng(23)
    terms = [rng.integers(0, 4, (tables[2 * m][0], tables[2 * m + 1][0])).astype(np.float64) for m in range(4)]
    at = lambda s, m: (s[2 * m] - tables[2 * m][1], s[2 * m + 1] - tables[2 * m + 1][1])  # noqa: E731
    # the seeded table, and a term that couples the ARM's weight step with the synthesis' so that a second sweep moves the ARM
    cost = lambda s: float(sum(terms[m][at(s, m)] for m in range(4))  # noqa: E731
                           + 4 * (abs((s[0] + 8) - (s[6] + 12) // 2) + 0.25 * (s[6] + 12 - 9) ** 2))
    still = lambda s: float(sum(v - f for v, f in zip(s, finest)))                                                # noqa: E731
    seen_one, seen_pair = [], []

    def price_one(m, steps):
        seen_one.append((m, tuple(steps)))
        return intra_tests._pricer(cost, lambda s: True, lambda s: 0)(m, steps)

    def price_pair(role, m, steps):
        if role == 0:
            seen_pair.append((m, tuple(steps[0])))
        assert steps[1] == finest
        return pair_tests._pricer(lambda s: cost(s[0]) + still(s[1]), lambda s: True, lambda s, role: 0)(role, m, steps)

    one, t_one = search_steps(price_one, has_ifce, 9)
    pair, t_pair = search_steps_pair(price_pair, (has_ifce, False), 9)
    per_sweep = 4 if has_ifce else 3
    assert seen_one == seen_pair and len(seen_one) >= 3 * per_sweep  # (at least: a sweep that moves, one more, the one that changes nothing)
    assert pair == [one, finest] and one != finest
    assert [(t.sweep, t.module, t.chosen) for t in t_one] == [(t.sweep, t.module, t.chosen) for t in t_pair if t.role == 0]
    assert [t.module for t in t_pair if t.role == 1][:3] == ["arm", "upsampling", "synthesis"] and all(t.chosen == 0 for t in t_pair if t.role == 1)
