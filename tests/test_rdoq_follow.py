"""RDOQ step whose claims follow the flows into the dependent frames (ccd_rdoq_follow, ccd_rdoq_set_dep_maps, RdoqStep.follow;
DESIGN.md section 4.17): a candidate of a reference R also claims, in the raster of every dependent F, the cells whose samples
can read what it changes.

CPU: the new entry points and the refusals that need no device; the numpy restatement (tests/rdoq_follow_ref.py) against itself -
the selected set of every truncation is pairwise disjoint in claim sets, the fixed point is the greedy walk in component key
order, n_open == 0 certifies maximality; and the implication the feature rests on, by brute force: claim sets without a common
cell => no sample of F has windows on both reference-change regions, or on one and in the other latent's footprint.
GPU: reach tables and flow boxes equal the restatement entry for entry; crafted offers that the step without follows selects
together; the settle lookup over three groups; seeded components for 1, 2, 3, 8 and 64 rounds; unrelated slots step as in a handle
without follows; flows rewritten in place; the refusals, also with a step in flight; tools/requantise_video.py --follow.  The
pick state of every latent is compared too (through ccd_rdoq_debug_picks).  Every comparison is in integers or bit-equal floats."""
import ctypes as C
import os

import numpy as np
import pytest

import rdoq_follow_ref as fr
from conftest import ROOT
from test_rdoq import ERR_ARG, SENTINEL, _compare, _device_outcome, _rects_meet, _Synth, _words, gpu  # noqa: F401  (gpu: the fixture)
from test_rdoq_rounds import _Crafted

ERR_VALUE = -2
NEW_ENTRY_POINTS = ["ccd_rdoq_follow", "ccd_rdoq_max_follows", "ccd_rdoq_set_dep_maps", "ccd_rdoq_slot_dep_sse", "ccd_rdoq_slot_reach",
                    "ccd_rdoq_slot_flow_boxes"]
FORMATS = {"rgb": "odd18x65", "yuv420": "yuv420_8b", "yuv444": "yuv444_8b"}
TAPS = (2, 4, 6, 8)


# ---- CPU -------------------------------------------------------------------------------------------------------------------------
def test_entry_points_and_refusals_without_a_device():
    from cool_chic_amd import RdoqStep, _lib, rdoq

    with open(os.path.join(ROOT, "include", "ccd.h")) as f:
        header = f.read()
    L = _lib.lib()
    for name in NEW_ENTRY_POINTS:
        assert name + "(" in header and name in _lib.SIGNATURES and getattr(L, name) is not None, name
    assert all(hasattr(RdoqStep, m) for m in ("follow", "set_dep_maps", "dep_sse", "reach", "flow_boxes"))
    assert rdoq.max_follows() == 4
    assert rdoq.StepResult._fields[-1] == "n_open" and len(rdoq.StepResult._fields) == 7  # dep_sse is an accessor
    handle = C.create_string_buffer(1024)  # stands for a handle: the calls must return before they look at it
    r = C.cast(handle, C.c_void_p)
    flows = np.zeros(16, np.float32)

    def desc(frame_type=1, which=0, motion=flows.ctypes.data, taps=8, target=1, frozen=-1):
        return _lib.RdoqFollow(frame_type, which, motion, (C.c_int32 * 4)(0, 0, 0, 0), taps, target, frozen)

    assert L.ccd_rdoq_follow(None, 0, C.byref(desc())) == ERR_ARG and L.ccd_rdoq_follow(r, 0, None) == ERR_ARG
    assert L.ccd_rdoq_follow(r, -1, C.byref(desc())) == ERR_ARG
    for bad in (dict(motion=None), dict(target=-1), dict(frozen=-2), dict(frame_type=0), dict(frame_type=3), dict(which=-1), dict(which=1),
                dict(frame_type=2, which=2)):
        assert L.ccd_rdoq_follow(r, 0, C.byref(desc(**bad))) == ERR_ARG, bad
    maps = (C.c_void_p * 4)()
    assert L.ccd_rdoq_set_dep_maps(None, 0, maps) == ERR_ARG and L.ccd_rdoq_set_dep_maps(r, -1, maps) == ERR_ARG
    v, dev = C.c_int64(7), C.c_void_p()
    assert L.ccd_rdoq_slot_dep_sse(None, 0, C.byref(v)) == ERR_ARG and L.ccd_rdoq_slot_dep_sse(r, 0, None) == ERR_ARG
    assert L.ccd_rdoq_slot_dep_sse(r, -1, C.byref(v)) == ERR_ARG and v.value == 7
    assert L.ccd_rdoq_slot_reach(None, 0, 0, C.byref(dev)) == ERR_ARG and L.ccd_rdoq_slot_reach(r, 0, 0, None) == ERR_ARG
    assert L.ccd_rdoq_slot_reach(r, -1, 0, C.byref(dev)) == ERR_ARG and L.ccd_rdoq_slot_reach(r, 0, -1, C.byref(dev)) == ERR_ARG
    assert L.ccd_rdoq_slot_flow_boxes(None, 0, 0, 0, C.byref(dev)) == ERR_ARG and L.ccd_rdoq_slot_flow_boxes(r, 0, 0, 0, None) == ERR_ARG
    for args in ((-1, 0, 0), (0, -1, 0), (0, 0, -1)):
        assert L.ccd_rdoq_slot_flow_boxes(r, *args, C.byref(dev)) == ERR_ARG
    assert not dev.value and bytes(handle) == bytes(1024)


def test_windows_restate_the_tap_intervals():
    """rdoq_follow_ref.windows is tests/test_dependent_deltas.py::_tap_interval (checked against the oracle there), sample by
    sample: 19 x 26, flows to +-30 so that the clamps occur."""
    h, w = 19, 26
    for taps in TAPS:
        rng = np.random.default_rng([taps, 417])
        motion = rng.uniform(-30.0, 30.0, size=(4, h, w)).astype(np.float32)
        gflow = [2, -3, -1, 4]
        for which in (0, 1):
            win = fr.windows(motion, which, taps, gflow)
            for y in range(h):
                for x in range(w):
                    want = fr._tap_interval(taps, motion[2 * which + 1, y, x], y, h, gflow[2 * which + 1]) + \
                        fr._tap_interval(taps, motion[2 * which, y, x], x, w, gflow[2 * which])
                    assert tuple(win[y, x]) == want, (taps, which, y, x)


def _sample_latents(g_, rng, n):
    """About n latents of the latent grids: anchors, their neighbours in the grid and the latents over the same place one grid up."""
    out = set()
    grids = [g for g in g_.lat_grids if g_.sizes[g] >= 4][:4]
    while len(out) < n:
        g = grids[int(rng.integers(len(grids)))]
        h, w = g_.hw[g]
        y, x = int(rng.integers(h)), int(rng.integers(w))
        for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2)):
            if y + dy < h and x + dx < w:
                out.add((g, y + dy, x + dx))
        if g + 1 in grids:
            out.add((g + 1, min(y // 2, g_.hw[g + 1][0] - 1), min(x // 2, g_.hw[g + 1][1] - 1)))
    return sorted(out)


def _cells(g_, boxes):
    """bool [n][cells]: the cells of each (top, left, bottom, right), empty boxes none."""
    out = np.zeros((len(boxes), g_.cells_h, g_.cells_w), bool)
    for i, (t, l, b, r) in enumerate(boxes):
        if t <= b:
            out[i, t:b + 1, l:r + 1] = True
    return out.reshape(len(boxes), -1)


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_disjoint_claim_sets_mean_no_common_sample(fmt):
    """The implication of DESIGN.md 4.17, by brute force over all pairs of ~150 sampled latents per case (> 10^4 pairs): P and B
    dependents (which 0 and 1), 2 / 4 / 6 / 8 taps, flows uniform in +-20 with a global flow (the border clamps occur)."""
    g_ = fr.geo(FORMATS[fmt])
    rng = np.random.default_rng([len(fmt), 419])
    n_disjoint = n_adjacent = n_residue = 0
    for which in (0, 1):
        for taps in TAPS:
            motion, gflow = fr.flows(g_, which + 1, 10 * taps + which)
            win = fr.windows(motion, which, taps, gflow)
            reach = fr.reach_table(win, g_.cells_h, g_.cells_w)
            lats = _sample_latents(g_, rng, 150)
            assert len(lats) * (len(lats) - 1) // 2 >= 10 ** 4
            own = [tuple(int(v) for v in g_.boxes()[g][y, x]) for g, y, x in lats]
            fbox = {g: fr.flow_boxes(reach, g_.boxes()[g]) for g in {l[0] for l in lats}}
            flow = [tuple(int(v) for v in fbox[g][y, x]) for g, y, x in lats]
            E = [fr.change_region(g_, g, y, x) for g, y, x in lats]
            foot = [g_.foot(g, y, x) for g, y, x in lats]
            hit = np.zeros((len(lats), g_.H, g_.W), bool)   # the samples of F with a window on E(p)
            inside = np.zeros((len(lats), g_.H, g_.W), bool)  # q's footprint as a latent of F's residue
            for i, e in enumerate(E):
                hit[i] = (win[..., 0] <= e[2]) & (win[..., 1] >= e[0]) & (win[..., 2] <= e[3]) & (win[..., 3] >= e[1])
                t, l, b, r = foot[i]
                if g_.fdt == 1:  # a chroma sample stands for its quad, in F as in the reference
                    q = hit[i].reshape(g_.H // 2, 2, g_.W // 2, 2).any(axis=(1, 3))
                    hit[i] = np.repeat(np.repeat(q, 2, axis=0), 2, axis=1)
                    t, l, b, r = t & ~1, l & ~1, b | 1, r | 1
                inside[i, t:b + 1, l:r + 1] = True
                # every sample that reads E(p) lies in a cell of p's flow box
                ys, xs = np.nonzero(hit[i])
                if len(ys):
                    assert flow[i][0] <= ys.min() // 8 and ys.max() // 8 <= flow[i][2] and flow[i][1] <= xs.min() // 8 and xs.max() // 8 <= flow[i][3]
            hit2, in2 = hit.reshape(len(lats), -1).astype(np.int32), inside.reshape(len(lats), -1).astype(np.int32)
            own_c, flow_c = _cells(g_, own).astype(np.int32), _cells(g_, flow).astype(np.int32)
            share_sample = (hit2 @ hit2.T) > 0
            share_foot = (hit2 @ in2.T) > 0           # [p][q]: a sample in q's footprint reads E(p)
            # both of R: the own boxes in R's raster, the flow boxes in F's
            meet = ((own_c @ own_c.T) > 0) | ((flow_c @ flow_c.T) > 0)
            off = ~np.eye(len(lats), dtype=bool)
            assert not (share_sample & ~meet & off).any(), (fmt, which, taps, np.argwhere(share_sample & ~meet & off)[:3].tolist())
            # p of R, q of F's residue: p's flow box and q's own box, both in F's raster
            meet_rf = (flow_c @ own_c.T) > 0
            assert not (share_foot & ~meet_rf).any(), (fmt, which, taps, np.argwhere(share_foot & ~meet_rf)[:3].tolist())
            n_disjoint += int((~meet & off).sum()) // 2
            n_residue += int((~meet_rf).sum())
            for i in range(len(lats)):
                for j in range(i + 1, len(lats)):
                    a, b = own[i], own[j]
                    grown = (a[0] - 1, a[1] - 1, a[2] + 1, a[3] + 1)
                    n_adjacent += _rects_meet(grown, b) and not _rects_meet(a, b)
    assert n_adjacent > 0, fmt
    if g_.cells_h * g_.cells_w > 100:  # (on 9 x 3 cells nearly every flow box of +-20 flows is the raster)
        assert n_disjoint > 1000 and n_residue > 1000, (fmt, n_disjoint, n_residue)


# ---- the components of the tests -------------------------------------------------------------------------------------------------
class _Component:
    """Slots 0, 1: two references R0, R1; slot 2: the residue of a B frame F that predicts from both (the leader of its pair),
    slot 3: F's motion cool-chic, linked to slot 2.  Follows: R0 -> 2 (which 0), R1 -> 2 (which 1), frozen 3.  All of one
    architecture; seeded maps, dependent maps on the references."""

    def __init__(self, name, seed=0, amplitude=20.0, taps=8, crafted=False):
        self.name, self.taps = name, taps
        self.g = fr.geo(name)
        self.motion, self.gflow = fr.flows(self.g, 2, seed, amplitude)
        if crafted:
            self.cases = [_Crafted(name) for _ in range(4)]
            self.syns = [c.syn for c in self.cases]
            for c, s in zip(self.cases, self.syns):
                s.lat, s.dd, s.db, s.kD, s.kR = c.lat, c.dd, c.db, 1.0, 1.0
            self.dep = [None] * 4
        else:
            self.syns = [fr.synth(name, seed + k) for k in range(4)]
            self.dep = [fr.dep_maps(self.syns[0], seed), fr.dep_maps(self.syns[1], seed + 1), None, None]
        self.reach = [fr.reach_table(fr.windows(self.motion, which, taps, self.gflow), self.g.cells_h, self.g.cells_w) for which in (0, 1)]
        self.handle = fr.Handle([self.g] * 4, links={3: 2}, follows=[(0, 2, self.reach[0]), (1, 2, self.reach[1])])
        # seeded maps: the fine grids, as RdEvaluator.descend advises (a coarse candidate with the best key owns the raster)
        self.masks = [(1 << self.g.n) - 1 if crafted else 7] * 3 + [0]

    def own(self, masks=None):
        masks = self.masks if masks is None else masks
        return [fr.own_cands(s, dep=self.dep[k], mask=masks[k]) for k, s in enumerate(self.syns)]

    def cands(self, masks=None):
        return self.handle.cands(self.own(masks))

    def device(self, gpu, extra=()):
        """(RdoqStep, fresh device copies of the slots [+ extra _Synth behind them], what keeps the device memory alive)."""
        import torch

        dev = [_Synth(self.name, 1).upload(s.lat, s.dd, s.db) for s in self.syns] + [e.upload() for e in extra]
        for d, s in zip(dev, self.syns):
            d.lat, d.kD, d.kR = s.lat, s.kD, s.kR
        step = gpu(0)
        for d in dev:
            d.add_to(step)
        step.link(3, 2)
        motion = torch.from_numpy(self.motion).cuda()
        for which in (0, 1):
            assert step.follow(which, 2, which, motion.data_ptr(), target=2, frozen=3, global_flow=self.gflow, warp_filter_size=self.taps,
                               owner=motion) == 0
        keep = [motion]
        for k, dep in enumerate(self.dep):
            if dep is not None:
                t = [torch.from_numpy(a).cuda() for a in dep]
                step.set_dep_maps(k, [a.data_ptr() for a in t], owner=t)
                keep.append(t)
        torch.cuda.synchronize()
        return step, dev, keep

    def run(self, step, dev, rounds, masks=None):
        masks = list(self.masks if masks is None else masks) + [(1 << d.geo.n) - 1 for d in dev[4:]]
        step.step([d.kD for d in dev], [d.kR for d in dev], [0.0] * len(dev), masks, rounds=rounds)
        step.wait()

    def compare(self, step, dev, rounds, what, masks=None):
        """The four slots against the restatement after `rounds` rounds; returns the Rounds."""
        own = self.own(masks)
        ref = fr.Rounds(self.handle, self.handle.cands(own), rounds)
        for k in range(4):
            s = self.syns[k]
            res, moves, after, raw = _device_outcome(step, k, dev[k])
            r = fr.slot_ref(self.handle, k, s.lat, own[k], ref.per_round)
            dep_want = sum(int(self.dep[k][g][(sg + 1) // 2, y, x]) for g, y, x, sg in r.chosen) if self.dep[k] is not None else 0
            dep_got = step.dep_sse(k)
            assert dep_got == dep_want, (what, k, dep_got, dep_want)
            assert res.d_cost == s.kD * float(res.d_sse + dep_got) + s.kR * res.d_bits, (what, k)
            res = res._replace(d_cost=s.kD * float(res.d_sse) + s.kR * res.d_bits)  # (_compare's form; d_sse is the OWN frame's)
            _compare(dev[k], (res, moves, after, raw), r, s.kD, s.kR, f"{what}, slot {k}, {rounds} rounds", s.dd, s.db)
            assert res.n_open == ref.n_open[k], (what, k, rounds, res.n_open, ref.n_open[k])
            # the pick state of every latent: 0 no candidate, 1 / 2 a candidate for -1 / +1, + 4 selected, + 8 blocked, neither: open
            want = [np.zeros(hw, np.uint8) for hw in self.g.hw]
            for state, group in ((0, self.handle.cands(own)), (4, ref.selected), (8, ref.blocked)):
                for _, slot, g, y, x, sg in group:
                    if slot == k:
                        want[g][y, x] = (1 if sg < 0 else 2) | state
            for g in range(self.g.n):
                got = _picks(step, k, g, self.g.hw[g])
                assert np.array_equal(got, want[g]), (what, k, g, rounds, np.argwhere(got != want[g])[:4].tolist())
        return ref


def _picks(step, slot, grid, hw):
    """The pick bytes of the last finished step (ccd_rdoq_debug_picks: exported for this test, not part of include/ccd.h)."""
    import torch

    from cool_chic_amd._handle import _DevArray
    from cool_chic_amd._lib import check, lib

    fn = lib().ccd_rdoq_debug_picks
    fn.restype, fn.argtypes = C.c_int64, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    ptr = C.c_void_p()
    assert check(fn(step._h, slot, grid, C.byref(ptr)), "ccd_rdoq_debug_picks") == hw[0] * hw[1]
    return torch.as_tensor(_DevArray(ptr.value, hw, "|u1", step), device="cuda").cpu().numpy()


_COMPONENTS = {}


def _component(*args, **kw):
    key = (args, tuple(sorted(kw.items())))
    if key not in _COMPONENTS:
        _COMPONENTS[key] = _Component(*args, **kw)
    return _COMPONENTS[key]


SEEDED = [("odd18x65", 20.0), ("yuv420_8b", 20.0), ("odd100x37", 3.0)]


@pytest.mark.parametrize("name,amplitude", SEEDED)
def test_the_rounds_over_claim_sets_end_at_the_greedy_walk(name, amplitude):
    """The restatement against itself on a component of three groups (four slots): every truncation is pairwise disjoint in
    claim sets, the fixed point is the walk in component key order, and n_open == 0 certifies that nothing can be added."""
    comp = _component(name, amplitude=amplitude)
    cands = comp.cands()
    assert len({c[1] for c in cands}) == 3 and len(cands) > 30  # the motion slot offers nothing
    assert sorted(c[0] & 0xFFFFFFFF for c in cands) == sorted({c[0] & 0xFFFFFFFF for c in cands})  # component-wide uids
    walk = fr.greedy(comp.handle, cands)
    seen, certified = 0, None
    for rounds in (1, 2, 3, 8, 64):
        ref = fr.Rounds(comp.handle, cands, rounds)
        sel = ref.selected
        assert len(sel) >= seen and set(sel) <= set(walk), (name, rounds)
        seen = len(sel)
        for i, a in enumerate(sel[:60]):
            for b in sel[i + 1:60]:
                assert not fr.claim_sets_meet(comp.handle, a, b), (name, rounds, a, b)
        if sum(ref.n_open) == 0:
            certified = certified or rounds
            assert set(sel) == set(walk), (name, rounds)
            chosen = set(sel)
            for c in cands[:200]:  # maximal: every other candidate meets a selected one
                assert c in chosen or any(fr.claim_sets_meet(comp.handle, c, s) for s in sel), (name, rounds, c)
    assert certified is not None and seen >= 2, (name, seen)
    # the follows matter: without them the same candidates give a larger set
    plain = fr.Rounds(fr.Handle([comp.g] * 4, links={3: 2}), cands, 64)
    assert len(plain.selected) > seen, (name, len(plain.selected), seen)


# Three coarse latents of odd100x37 (grid 3: own boxes of 35 .. 65 of the 65 cells, a wave's), one per raster of the component.  The
# reference of slot 0 has the best key; the one of slot 1 meets it in F's raster alone, through the two flow boxes; F's own
# latent meets its flow box with its own box.
WAVE_OFFERS = [(0, 3, 2, 6, -1000), (1, 3, 2, 6, -100), (2, 3, 2, 6, -50)]


def _place(comp, offers):
    """offers: [(slot, g, y, x, cost)] as the only candidates of a crafted component."""
    for c in comp.cases:
        c.dd = [np.full_like(a, SENTINEL) for a in c.dd]
        c.syn.dd = c.dd
    for slot, g, y, x, cost in offers:
        comp.cases[slot].offer(g, y, x, cost)


def test_the_cases_reach_every_route_of_the_step():
    """A condition on the inputs of the GPU tests below, not a measurement: the device walks an own box of up to 32 cells in its
    latent's lane and a larger one in a wave, and either can be blocked by a taken cell of the own box or of a flow box alone,
    lose a select through a cell of the own box or of a flow box alone, or be selected.  The seeded components (8 rounds) and
    the crafted waves (3 rounds) together hold a candidate for every one of the ten."""
    from cool_chic_amd._lib import lib

    assert lib().ccd_rdoq_lane_cells() == fr.LANE_CELLS  # the threshold the restatement sorts lane from wave by is the device's
    seen = {}
    for name, amplitude in SEEDED:
        comp = _component(name, amplitude=amplitude)
        for route, cands in fr.decisions(comp.handle, comp.cands(), 8).items():
            seen[route] = seen.get(route, 0) + len(cands)
    lanes_alone = dict(seen)
    comp = _component("odd100x37", amplitude=3.0, crafted=True)
    _place(comp, WAVE_OFFERS)
    for route, cands in fr.decisions(comp.handle, comp.cands(), 3).items():
        seen[route] = seen.get(route, 0) + len(cands)
    for wave in (False, True):
        for what in fr.DECISIONS:
            assert seen.get((wave, what), 0) > 0, (wave, what, seen)
    assert all(lanes_alone.get((False, what), 0) > 0 for what in fr.DECISIONS), lanes_alone  # (odd18x65 has no wave's box at all)


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
def _np(dev_array):
    import torch

    return torch.as_tensor(dev_array, device="cuda").cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_reach_tables_and_flow_boxes(gpu, fmt):
    """P and B dependents (which 0 and 1), 2 / 4 / 6 / 8 taps, flows uniform in +-20 with a global flow: the reach table of every
    follow equals the restatement entry for entry, empties included, and so do the flow boxes of every latent of every grid."""
    import torch

    g_ = fr.geo(FORMATS[fmt])
    syns = [_Synth(g_.name, k).upload() for k in range(3)]
    step = gpu(0)
    for s in syns:
        s.add_to(step)
    want, keep = {}, []
    for which in (0, 1):
        for k, taps in enumerate(TAPS):
            motion, gflow = fr.flows(g_, which + 1, 10 * taps + which)
            if taps == 8 and which == 0:  # a corner nobody reads: the flows of the whole frame point far to the bottom right
                motion[:] = np.abs(motion) + 24.0
            t = torch.from_numpy(motion).cuda()
            keep.append(t)
            assert step.follow(which, which + 1, which, t.data_ptr(), target=2, global_flow=gflow, warp_filter_size=taps) == k
            want[which, k] = fr.reach_table(fr.windows(motion, which, taps, gflow), g_.cells_h, g_.cells_w)
    torch.cuda.synchronize()
    step.step([1.0] * 3, [1.0] * 3, [0.0] * 3, [0] * 3)  # nothing may move; the tables are built all the same
    step.wait()
    n_empty = 0
    for (slot, k), ref in want.items():
        words = _np(step.reach(slot, k))
        assert words.dtype == np.uint32 and words.shape == (g_.cells_h, g_.cells_w, 4)
        got = fr.reach_from_device(words)
        assert np.array_equal(got, ref), (fmt, slot, k, np.argwhere((got != ref).any(axis=-1))[:4].tolist())
        n_empty += int((ref[..., 0] < 0).sum())
        for g in range(g_.n):
            fb = _np(step.flow_boxes(slot, k, g)).astype(np.int64)
            ref_fb = fr.flow_boxes(ref, g_.boxes()[g])
            assert fb.shape == g_.hw[g] + (4,) and np.array_equal(fb, ref_fb), (fmt, slot, k, g, np.argwhere((fb != ref_fb).any(axis=-1))[:4].tolist())
    assert n_empty > 0, fmt
    assert all(step.result(s).n_moves == 0 for s in range(3))
    step.close()


def _find(comp, cond, slots, grids=(0, 1)):
    """The first pair of latents (slot, g, y, x) of the two slots, on a coarse lattice, that `cond` accepts."""
    g_ = comp.g
    pts = [(g, y, x) for g in grids for y in range(0, g_.hw[g][0], 3) for x in range(0, g_.hw[g][1], 2)]
    for a in pts:
        for b in pts:
            if (slots[0], a) != (slots[1], b) and cond((0, slots[0]) + a + (-1,), (0, slots[1]) + b + (-1,)):
                return a, b
    raise AssertionError("no such pair")


def _crafted_step(gpu, comp, offers, rounds_list, what, masks=None):
    """offers: [(slot, g, y, x, cost)].  One fresh handle per number of rounds; returns {rounds: Rounds}."""
    _place(comp, offers)
    out = {}
    for rounds in rounds_list:
        step, dev, keep = comp.device(gpu)
        comp.run(step, dev, rounds, masks)
        out[rounds] = comp.compare(step, dev, rounds, what, masks)
        step.close()
    return out


@pytest.mark.gpu
def test_crafted_offers_meet_through_the_flows(gpu):
    """Offers that a step without follows selects together (their own boxes share no cell, or lie in different rasters) and that
    meet in F's raster: round 1 selects only the smaller key, round 2 blocks the other."""
    comp = _component("odd18x65", amplitude=20.0, crafted=True)
    H = comp.handle
    plain = fr.Handle([comp.g] * 4, links={3: 2})

    def meets_only_through_flows(a, b):
        return not fr.claim_sets_meet(plain, a, b) and fr.claim_sets_meet(H, a, b)

    cases = {
        "two latents of R": (0, 0),           # disjoint own boxes, flow boxes that share a cell of F
        "R against F's residue": (0, 2),      # the residue latent's box lies in R's flow box
        "two references of one B frame": (0, 1),
    }
    for what, slots in cases.items():
        a, b = _find(comp, meets_only_through_flows, slots)
        offers = [(slots[0],) + a + (-100,), (slots[1],) + b + (-50,)]
        res = _crafted_step(gpu, comp, offers, (1, 2), what)
        first, second = res[1], res[2]
        assert [(c[1],) + c[2:5] for c in first.selected] == [(slots[0],) + a], what   # only the smaller key
        assert sum(first.n_open) == 1
        assert len(second.selected) == 1 and sum(second.n_open) == 0 and [(c[1],) + c[2:5] for c in second.blocked] == [(slots[1],) + b], what
        # without follows both are selected at once: what the step did before claims followed the flows
        assert len(fr.Rounds(plain, comp.cands(), 1).selected) == 2, what


@pytest.mark.gpu
def test_crafted_waves_take_every_route(gpu):
    """WAVE_OFFERS on odd100x37, the smallest fixture whose coarse latents have a wave's box: round 1 selects the wave of slot 0;
    the wave of slot 1 loses through its flow box alone and the wave of slot 2 through its own box, and round 2 blocks them the
    same way.  Every route of a wave through claim and select, against the restatement for 1, 2 and 3 rounds."""
    comp = _component("odd100x37", amplitude=3.0, crafted=True)
    res = _crafted_step(gpu, comp, WAVE_OFFERS, (1, 2, 3), "waves")
    routes = fr.decisions(comp.handle, comp.cands(), 3)
    assert {route: [c[1] for c in cands] for route, cands in routes.items()} == {
        (True, "selected"): [0], (True, "lost, flow box only"): [1], (True, "lost, own box"): [2],
        (True, "blocked, flow box only"): [1], (True, "blocked, own box"): [2]}
    assert [c[1] for c in res[1].selected] == [0] and res[1].n_open == (0, 1, 1, 0)
    for rounds in (2, 3):
        assert [c[1] for c in res[rounds].selected] == [0] and sorted(c[1] for c in res[rounds].blocked) == [1, 2] and sum(res[rounds].n_open) == 0


@pytest.mark.gpu
def test_settle_finds_owners_across_three_groups(gpu):
    """The strongest offer on a uid boundary of a component of three groups - the last latent of slot 0, the first of slot 1, the
    first of slot 2 - and weaker offers around it in every slot: the boundary owner is selected in round 1, and rounds >= 2 block
    exactly what the restatement blocks, which they can only if settle looks the owner up in the right slot."""
    comp = _component("odd18x65", amplitude=3.0, crafted=True)
    g_ = comp.g
    n, last = sum(g_.sizes), g_.n - 1
    lat0 = g_.lat_grids[0]
    h0, w0 = g_.hw[lat0]
    rng = np.random.default_rng(420)
    weaker = [(slot, lat0, int(rng.integers(h0)), int(rng.integers(w0)), -int(rng.integers(1, 500))) for slot in (0, 1, 2) for _ in range(40)]
    weaker = [o for o in weaker if o[2:4] != (0, 0)]
    for owner, uid in (((0, last, g_.hw[last][0] - 1, g_.hw[last][1] - 1), n - 1), ((1, 0, 0, 0), n), ((2, 0, 0, 0), 2 * n)):
        res = _crafted_step(gpu, comp, [owner + (-900,)] + weaker, (1, 2, 3), f"owner {uid}")
        assert uid in {c[0] & 0xFFFFFFFF for c in res[1].selected}, uid
        assert len(res[3].blocked) >= 1 and len(res[3].blocked) == len(res[2].blocked) + sum(1 for c in res[3].blocked if c not in res[2].blocked)
        if uid != n - 1:  # (the coarsest latent's box is the raster: it blocks everything)
            assert len(res[3].selected) > len(res[1].selected), uid


@pytest.mark.gpu
@pytest.mark.parametrize("name,amplitude", SEEDED)
def test_seeded_components(gpu, name, amplitude):
    """Seeded own, dependent and rate maps on the component of _Component, beside two slots in no follow relation: moves,
    latents, candidates, n_open, d_sse, dep_sse and d_bits equal the restatement for 1, 2, 3, 8 and 64 rounds; the unrelated
    slots step as in a handle that has no follows at all; and a second call leaves the same words."""
    comp = _component(name, amplitude=amplitude)
    others = ["rgb192", "odd18x65"]
    words = {}
    for rounds in (1, 2, 3, 8, 64):
        step, dev, keep = comp.device(gpu, extra=[_Synth(n, 7) for n in others])
        comp.run(step, dev, rounds)
        ref = comp.compare(step, dev, rounds, name)
        words[rounds] = [_words(_device_outcome(step, k, dev[k])) + (step.dep_sse(k),) for k in range(6)]
        assert step.dep_sse(4) == 0 and step.dep_sse(5) == 0
        step.close()
        if rounds == 8:
            assert len(ref.selected) >= 2 and any(comp.dep[c[1]] is not None for c in ref.selected)
        if rounds in (1, 8):
            plain = gpu(0)  # no follows, no dependent maps: the kernels every handle ran before
            alone = [_Synth(n, 7).upload() for n in others]
            for s in alone:
                s.add_to(plain)
            plain.step([s.kD for s in alone], [s.kR for s in alone], [0.0] * 2, [(1 << s.geo.n) - 1 for s in alone], rounds=rounds)
            plain.wait()
            for k, s in enumerate(alone):
                assert _words(_device_outcome(plain, k, s)) == words[rounds][4 + k][:-1], (name, rounds, k)
            plain.close()
            step, dev, keep = comp.device(gpu)  # again, without the other slots
            comp.run(step, dev, rounds)
            assert [_words(_device_outcome(step, k, dev[k])) + (step.dep_sse(k),) for k in range(4)] == words[rounds][:4], (name, rounds)
            step.close()


@pytest.mark.gpu
def test_flows_rewritten_in_place_are_followed(gpu):
    """Two steps of one handle; between them the flows are rewritten in the motion output the follows point at and the latents
    are put back: the second step's reach tables, flow boxes and selection are those of the new flows."""
    import torch

    comp = _component("odd18x65", amplitude=3.0)
    step, dev, keep = comp.device(gpu)
    comp.run(step, dev, 8)
    first = comp.compare(step, dev, 8, "first flows")
    assert np.array_equal(fr.reach_from_device(_np(step.reach(0, 0))), comp.reach[0])
    other = _Component("odd18x65", seed=5, amplitude=20.0)
    keep[0].copy_(torch.from_numpy(other.motion))  # (the same global flow would be a coincidence: the follow keeps the first one's)
    for d in dev:
        d.buf.copy_(torch.from_numpy(d.host_buffer(d.lat).view(np.int8)))
    torch.cuda.synchronize()
    reach = [fr.reach_table(fr.windows(other.motion, which, comp.taps, comp.gflow), comp.g.cells_h, comp.g.cells_w) for which in (0, 1)]
    saved = list(comp.handle.follows)
    try:
        for which in (0, 1):
            comp.handle.set_reach(which, 0, reach[which])
        comp.run(step, dev, 8)
        second = comp.compare(step, dev, 8, "rewritten flows")
        for which in (0, 1):
            assert np.array_equal(fr.reach_from_device(_np(step.reach(which, 0))), reach[which])
            assert np.array_equal(_np(step.flow_boxes(which, 0, 0)).astype(np.int64), comp.handle.flow_box(which, 0, 0))
    finally:
        comp.handle.follows = saved
        comp.handle._fbox = {}
    assert {c[:5] for c in first.selected} != {c[:5] for c in second.selected}
    step.close()


@pytest.mark.gpu
def test_refusals_on_a_live_handle(gpu):
    """Slots 0 - 3: the component; 4: rgb192 (another size); 5: odd18x65 added as yuv444 (another frame_data_type).
    CCD_ERR_VALUE for a frozen slot that may move (latents untouched), target == slot, a filter size the warp refuses, a target of
    another img_size and one of another frame_data_type; CCD_ERR_ARG for slots past the handle, a fifth follow and, for every new
    call, a step in flight.  A refused call leaves the handle as it was: the step around the refusals in flight and the step after
    them are the restatement's, word for word the same."""
    import torch

    from cool_chic_amd._lib import CcdError, RdoqFollow, lib

    L = lib()
    comp = _component("odd18x65", amplitude=3.0)
    step, dev, keep = comp.device(gpu, extra=[_Synth("rgb192", 7)])
    odd = _Synth("odd18x65", 2).upload()
    assert step.add(odd.geo.arch, 2, [odd.buf.data_ptr() + p for p in odd.pos], owner=odd.buf) == 5
    step.set_maps(5, [t.data_ptr() for t in odd.dd_dev], [t.data_ptr() for t in odd.db_dev], owner=(odd.dd_dev, odd.db_dev))
    dev.append(odd)
    h, motion = step._h, keep[0]

    def desc(which=0, taps=8, target=2, frozen=-1):
        return RdoqFollow(2, which, motion.data_ptr(), (C.c_int32 * 4)(0, 0, 0, 0), taps, target, frozen)

    assert L.ccd_rdoq_follow(h, 0, C.byref(desc(target=0))) == ERR_VALUE
    for taps in (0, 3, 18):
        assert L.ccd_rdoq_follow(h, 0, C.byref(desc(taps=taps))) == ERR_VALUE
    assert L.ccd_rdoq_follow(h, 0, C.byref(desc(target=4))) == ERR_VALUE  # rgb192 is another picture
    assert L.ccd_rdoq_follow(h, 0, C.byref(desc(target=5))) == ERR_VALUE and L.ccd_rdoq_follow(h, 5, C.byref(desc())) == ERR_VALUE  # frame_data_type
    assert L.ccd_rdoq_follow(h, 6, C.byref(desc())) == ERR_ARG and L.ccd_rdoq_follow(h, 0, C.byref(desc(target=6))) == ERR_ARG
    assert L.ccd_rdoq_follow(h, 0, C.byref(desc(frozen=6))) == ERR_ARG
    dev_ptr, v = C.c_void_p(), C.c_int64(7)
    assert L.ccd_rdoq_slot_reach(h, 0, 0, C.byref(dev_ptr)) == ERR_ARG and not dev_ptr.value  # no step yet
    before = [d.buf.cpu().numpy().copy() for d in dev]
    masks = list(comp.masks) + [1, 1]
    masks[3] = 1  # the motion cool-chic of the followed frame may move: refused before anything is enqueued
    with pytest.raises(CcdError) as e:
        step.step([d.kD for d in dev], [d.kR for d in dev], [0.0] * 6, masks, rounds=2)
    assert e.value.code == ERR_VALUE
    step.wait()
    assert all(np.array_equal(d.buf.cpu().numpy(), b) for d, b in zip(dev, before))

    def enqueue():
        step.step([d.kD for d in dev], [d.kR for d in dev], [0.0] * 6, list(comp.masks) + [(1 << d.geo.n) - 1 for d in dev[4:]], rounds=2)

    def words():
        return [_words(_device_outcome(step, k, d)) + (step.dep_sse(k), step.result(k).n_open) for k, d in enumerate(dev)]

    # a step in flight: every new call is refused, and the step is the one a handle nobody disturbed runs
    enqueue()
    maps = (C.c_void_p * comp.g.n)()
    assert L.ccd_rdoq_follow(h, 0, C.byref(desc())) == ERR_ARG
    assert L.ccd_rdoq_set_dep_maps(h, 2, maps) == ERR_ARG and L.ccd_rdoq_set_dep_maps(h, 0, None) == ERR_ARG
    assert L.ccd_rdoq_slot_dep_sse(h, 0, C.byref(v)) == ERR_ARG and v.value == 7
    assert L.ccd_rdoq_slot_reach(h, 0, 0, C.byref(dev_ptr)) == ERR_ARG and L.ccd_rdoq_slot_flow_boxes(h, 0, 0, 0, C.byref(dev_ptr)) == ERR_ARG
    assert not dev_ptr.value
    step.wait()
    comp.compare(step, dev, 2, "around the refusals in flight")
    want = words()
    assert any(w[-2] != 0 for w in want[:2])  # (the dependent maps are still set: the refused set_dep_maps(0, NULL) took nothing away)
    assert L.ccd_rdoq_slot_reach(h, 0, 0, C.byref(dev_ptr)) == comp.g.cells_h * comp.g.cells_w and dev_ptr.value
    assert L.ccd_rdoq_slot_reach(h, 0, 1, C.byref(dev_ptr)) == ERR_ARG  # slot 0 has one follow
    for d in dev:  # ... and once more after them, from the latents as they were
        d.buf.copy_(torch.from_numpy(d.host_buffer(d.lat).view(np.int8)))
    torch.cuda.synchronize()
    enqueue()
    step.wait()
    comp.compare(step, dev, 2, "after the refusals")
    assert words() == want
    for k in range(1, 4):
        assert L.ccd_rdoq_follow(h, 0, C.byref(desc())) == k
    assert L.ccd_rdoq_follow(h, 0, C.byref(desc())) == ERR_ARG  # a fifth
    assert L.ccd_rdoq_slot_reach(h, 0, 1, C.byref(dev_ptr)) == ERR_ARG  # no finished step covered the new follows
    torch.cuda.synchronize()
    step.close()


@pytest.mark.gpu
def test_requantise_video_tool_follow(gpu, tmp_path):
    """tools/requantise_video.py --follow --rounds 8 --max-steps 2 --grids 0,1,2 on the stream and source of
    tests/test_rdoq_joint.py::test_requantise_video_tool_joint: the I frame of vid3_ldp descends together with the residue of
    the P frame that predicts from it.  Exit status 0 (the tool asserts that what it wrote decodes to the planes it scored), the
    joint descent is reported and moved something, the output parses, and its per-frame costs sum to no more than the input's."""
    import subprocess
    import sys

    import torch

    import inter_cases as ic
    from conftest import GOLDEN
    from cool_chic_amd import DecodeBatch
    from cool_chic_amd.bitstream.decode import _split_frame, decode_video
    from cool_chic_amd.bitstream.header import VideoHeader

    lmbda = 1e-3
    fh, ((arch, hdr, nn, lat),), _, _ = ic.parse_video("vid3_ldp")[0]
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
                          "--max-steps", "2", "--grids", "0,1,2", "--rounds", "8", "--follow"], cwd=ROOT, capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stderr[-2000:]
    first = next(line for line in run.stdout.splitlines() if line.startswith("frame 0 (I)"))
    assert "intra + residues of 1" in first and "after:" in run.stdout
    n_intra, n_res = (int(v) for v in first.split("steps ")[1].split(" intra")[0].split(" + "))
    assert n_intra >= 1 and n_res >= 1, first

    def costs(path):
        with open(path, "rb") as f:
            rest = VideoHeader().read_header(f.read())
        frames = decode_video(path)
        total = []
        for k in range(3):  # vid3_ldp: coding order = display order
            n0 = len(rest)
            _, ccs, rest = _split_frame(rest)
            planes = frames[str(k)].integer_planes()
            sse = sum(int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum()) for a, b in zip(planes, sources[k]))
            total.append(sse / (sum(a.size for a in planes) * 255.0 * 255.0) + lmbda * 8.0 * (n0 - len(rest)) / (128 * 224))
        assert rest == b""
        return total

    before, after = costs(src), costs(out)
    print("cost per frame before", before, "after", after)
    assert sum(after) <= sum(before)


@pytest.mark.gpu
def test_gop_step_end_to_end(gpu):
    """Depth one: two intra candidates (vid5's I frame from two latent sets), a B frame that predicts from both and a P frame on
    the first (vid5's coding indices 2 and 1 over the candidates' planes).  One GopDescent.step with rounds=8 on the fine grids:
    the summed SSE of the four frames, measured again by the evaluators' QualityMeter after the step, is before + sum d_sse +
    sum dep_sse exactly, and a moved reference latent has a non-zero dependent entry - own deltas alone would not add up."""
    import torch

    import dependent_cases as dc
    import inter_cases as ic
    from cool_chic_amd import InterRdEvaluator
    from cool_chic_amd.rd import RdEvaluator
    from cool_chic_amd.rd_gop import GopDescent
    from test_inter_deltas import _frame_data

    refs = [dc.intra("vid5", 0, seed=k) for k in (0, 1)]
    frames = [(ic.case("vid5", 2), [0, 1], [0, -2, 1, 3]), (ic.case("vid5", 1), [0], [1, -1, 0, 0])]
    lmbda = 1e-3
    lat = [r.cc.lat_dev.clone() for r in refs]
    flat = [{role: c.cc[role].lat_dev.clone() for role in ic.ROLES} for c, _, _ in frames]
    with RdEvaluator(0) as intra, InterRdEvaluator(0) as inter, GopDescent(intra, inter) as gop:
        for r, dev in zip(refs, lat):
            intra.add(r.arch, r.nn, r.cc.ptrs(dev), _frame_data(r.src, r.bd, r.fdt), owner=dev)
        for (c, which, gflow), dev in zip(frames, flat):
            inter.add(c.frame_type, *[(c.cc[role].arch, c.cc[role].nn, c.cc[role].ptrs(dev[role])) for role in ic.ROLES],
                      [gop.reference_planes(k) for k in which], gflow, c.taps, _frame_data(c.src, c.bd, c.fdt), owner=dev)
        for f, (c, which, _) in enumerate(frames):
            for w, k in enumerate(which):
                gop.follow(k, f, w)
        with pytest.raises(ValueError):
            gop.follow(1, 1, 0)  # the P frame predicts from candidate 0
        before = [t.clone() for t in lat] + [d["residue"].clone() for d in flat] + [d["motion"].clone() for d in flat]
        rep = gop.step(lmbda, grids=(0, 1, 2), rounds=8)
        after_i, after_f = intra.evaluate(lmbda), inter.evaluate(lmbda)
        sse0 = sum(sum(int(v) for v in c.quality.sse) for c in rep.intra + rep.inter)
        sse1 = sum(sum(int(v) for v in c.quality.sse) for c in after_i + after_f)
        for s in rep.slots:
            print(f"{s.role} {s.frame}: {s.step.n_candidates} candidates, {s.step.n_moves} moves, {s.step.n_open} open, d_sse {s.d_sse}, "
                  f"dep_sse {s.dep_sse}, d_bits {s.d_bits:.2f}")
        print("summed SSE", sse0, "->", sse1, "predicted", rep.d_sse)
        assert sse1 - sse0 == rep.d_sse == sum(s.d_sse + s.dep_sse for s in rep.slots)
        moved = [int((a != b).sum()) for a, b in zip(lat + [d["residue"] for d in flat] + [d["motion"] for d in flat], before)]
        assert moved[:4] == [s.step.n_moves for s in (rep.slots[0], rep.slots[1], rep.slots[2], rep.slots[4])] and moved[4:] == [0, 0]
        assert min(moved[:4]) >= 1, moved  # every intra candidate and both residues moved
        assert all(s.dep_sse == 0 for s in rep.slots[2:]) and all(s.step.n_moves == 0 for s in rep.slots if s.role == "motion")
        n_dep = 0
        for k in range(2):  # a moved reference latent with a non-zero dependent entry
            for g in range(3):
                mv = torch.as_tensor(gop.step_moves(k, "intra", g), device="cuda").cpu().numpy()
                dep = torch.as_tensor(intra.dependent_delta_map(k, g), device="cuda").cpu().numpy()
                ys, xs = np.nonzero(mv)
                n_dep += sum(1 for y, x in zip(ys, xs) if dep[(mv[y, x] + 1) // 2, y, x] != 0)
        assert n_dep >= 1 and any(s.dep_sse != 0 for s in rep.slots[:2])
        # own deltas alone do not add up
        assert sse1 - sse0 != sum(s.d_sse for s in rep.slots)
