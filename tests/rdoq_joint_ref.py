"""Helpers of tests/test_rdoq_joint.py: the rounds of an RDOQ step restated in numpy for a linked PAIR of slots (ccd_rdoq_link;
DESIGN.md section 4.14, "Groups") - two geometries on one raster of cells, keys with the group-wide index, boxes from
ccd_rdoq_influence_box - and the geometries, seeded maps and crafted offers the tests run on.

A candidate of a pair is (key, slot, g, y, x, s): slot 0 is the leader, slot 1 the follower, and the follower's keys are its own
slot's keys plus the number of the leader's latents."""
import numpy as np

import test_rdoq
from test_rdoq import _Geo, _geo, _rects_meet, _reference_step, _Synth  # noqa: F401  (_rects_meet: for the tests)
from test_rdoq_rounds import ONES, _as_ref, _Crafted


# ---- geometries ------------------------------------------------------------------------------------------------------------------
class _ArchGeo(_Geo):
    """What _Synth, _reference_step and _compare read of a tests/test_rdoq.py::_Geo, for an architecture that is given (a cool-chic
    of a video fixture) rather than looked up by the name of an image fixture."""

    def __init__(self, name, arch, nn, bd, fdt):
        from cool_chic_amd import rdoq

        self.name, self.arch, self.nn, self.bd, self.fdt = name, arch, nn, bd, fdt
        self.n = int(arch.n_grids)
        self.hw = [(int(arch.grid_h[g]), int(arch.grid_w[g])) for g in range(self.n)]
        self.sizes = [h * w for h, w in self.hw]
        self.first = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.H, self.W = int(arch.img_size[0]), int(arch.img_size[1])
        self.cell = rdoq.cell()
        self.cells_h, self.cells_w = -(-self.H // self.cell), -(-self.W // self.cell)
        self.hyper = [bool(arch.is_hyperlatent[g]) for g in range(self.n)]
        self._boxes = None


VIDEO = {"vid3_ldp_residue": 0, "vid3_ldp_motion": 1}


def geo(name):
    """_geo(name) of tests/test_rdoq.py; the two cool-chics of vid3_ldp frame 1 under the names of VIDEO (registered with _geo's
    cache, so that _Synth(name) finds them)."""
    if name in VIDEO and name not in test_rdoq._GEO:
        import inter_cases as ic

        fh, ccs, _, _ = ic.parse_video("vid3_ldp")[1]
        arch, _, nn, _ = ccs[VIDEO[name]]
        test_rdoq._GEO[name] = _ArchGeo(name, arch, nn, int(fh.bitdepth), int(fh.frame_data_type))
    return _geo(name)


# (leader: name, seed), (follower: name, seed).  The seeds are chosen on the CPU (test_the_cases_are_honest prints what each pair gives).
PAIRS = {
    "odd18x65": (("odd18x65", 0), ("odd18x65", 1)),
    "yuv420_8b": (("yuv420_8b", 0), ("yuv420_8b", 1)),
    "vid3_ldp": (("vid3_ldp_residue", 0), ("vid3_ldp_motion", 1)),
}


class Pair:
    """Two geometries on one raster."""

    def __init__(self, lead, foll):
        assert (lead.cells_h, lead.cells_w, lead.H, lead.W, lead.fdt) == (foll.cells_h, foll.cells_w, foll.H, foll.W, foll.fdt)
        self.geos = (lead, foll)
        self.cells_h, self.cells_w = lead.cells_h, lead.cells_w
        self.offset = (0, int(sum(lead.sizes)))  # what a slot's own uid becomes in the group
        assert self.offset[1] + sum(foll.sizes) < 2 ** 32

    def box(self, c):
        t, l, b, r = self.geos[c[1]].boxes()[c[2]][c[3], c[4]]
        return slice(t, b + 1), slice(l, r + 1)

    def cands(self, per_slot):
        """per_slot[k]: [(key, g, y, x, s)] as _reference_step lists a slot's own candidates."""
        return [(key + self.offset[k], k, g, y, x, s) for k in range(2) for key, g, y, x, s in per_slot[k]]


class Rounds:
    """`max_rounds` rounds over the candidates of a pair.  per_round: the winners of each round; n_open[k]: the candidates of slot k
    that took part in the last round without being selected; lost_to: {(slot of a loser, slot of the candidate that holds one of its
    cells)}; blocked_by: {(slot of a candidate blocked in round >= 2, slot of the selected candidate that owns one of its cells)}."""

    def __init__(self, pair, cands, max_rounds):
        taken = np.zeros((pair.cells_h, pair.cells_w), bool)
        owner = np.full((pair.cells_h, pair.cells_w), -1, np.int64)  # the slot whose selected candidate took the cell
        open_, self.per_round, self.lost_to, self.blocked_by = list(cands), [], set(), set()
        slot_of = {c[0]: c[1] for c in cands}
        for _ in range(max_rounds):
            if not open_:  # nothing left to compete: the remaining rounds select nothing and leave nothing open
                self.per_round.append([])
                continue
            for c in open_:                                               # 1. blocked for good
                if taken[pair.box(c)].any():
                    self.blocked_by |= {(c[1], int(k)) for k in np.unique(owner[pair.box(c)]) if k >= 0}
            open_ = [c for c in open_ if not taken[pair.box(c)].any()]
            raster = np.full((pair.cells_h, pair.cells_w), ONES, np.uint64)
            for c in open_:                                               # 2. claim
                np.minimum(raster[pair.box(c)], np.uint64(c[0]), out=raster[pair.box(c)])
            won = [c for c in open_ if (raster[pair.box(c)] == np.uint64(c[0])).all()]  # 3. select
            for c in open_:
                self.lost_to |= {(c[1], slot_of[int(k)]) for k in np.unique(raster[pair.box(c)]) if int(k) != c[0]}
            for c in won:                                                 # 4. their cells are taken
                taken[pair.box(c)] = True
                owner[pair.box(c)] = c[1]
            won_keys = {c[0] for c in won}
            open_ = [c for c in open_ if c[0] not in won_keys]
            self.per_round.append(won)
        self.n_open = tuple(sum(1 for c in open_ if c[1] == k) for k in range(2))
        self.selected = [c for won in self.per_round for c in won]


def greedy(pair, cands):
    """The walk over the pair's candidates in ascending key order: a candidate is taken unless its box holds a taken cell."""
    taken = np.zeros((pair.cells_h, pair.cells_w), bool)
    out = []
    for c in sorted(cands):
        if not taken[pair.box(c)].any():
            taken[pair.box(c)] = True
            out.append(c)
    return out


def fixed_point(pair, cands):
    """(the rounds up to and including the last one that selects, rounds until nothing is open)."""
    full = Rounds(pair, cands, 64)
    n_sel = max((k + 1 for k, w in enumerate(full.per_round) if w), default=0)
    n_certified = next(r for r in range(1, 66) if Rounds(pair, cands, r).n_open == (0, 0))
    return full.per_round[:n_sel], n_certified


def slot_ref(pair, k, lat, slot_cands, per_round):
    """The tests/test_rdoq.py::_Ref of slot k of a step that selected `per_round`."""
    return _as_ref(pair.geos[k], lat, slot_cands, [[(key - pair.offset[1] * k, g, y, x, s) for key, slot, g, y, x, s in won if slot == k]
                                                   for won in per_round])


# ---- seeded maps -----------------------------------------------------------------------------------------------------------------
_SEEDED = {}


def seeded(label, masks=None):
    """(Pair, the two _Synth (host side), each slot's own candidates under `masks` (all grids by default), the pair's candidates);
    once per label and masks."""
    key = (label, masks)
    if key not in _SEEDED:
        syns = [_Synth(geo(name).name, seed) for name, seed in PAIRS[label]]
        pair = Pair(syns[0].geo, syns[1].geo)
        own = [_reference_step(s.geo, s.lat, s.dd, s.db, s.kD, s.kR, 0.0, (1 << s.geo.n) - 1 if masks is None else masks[k]).cands
               for k, s in enumerate(syns)]
        _SEEDED[key] = (pair, syns, own, pair.cands(own))
    return _SEEDED[key]


def fresh(label):
    """The pair's two _Synth on the device, buffers of their own."""
    return [_Synth(geo(name).name, seed).upload() for name, seed in PAIRS[label]]


# ---- crafted offers --------------------------------------------------------------------------------------------------------------
class CraftedPair:
    """Two tests/test_rdoq_rounds.py::_Crafted of one architecture, leader and follower: no move anywhere except where a case
    offers one (costs kD = kR = 1, so the cost of an offer is its dD)."""

    def __init__(self, name):
        geo(name)
        self.cases = (_Crafted(name), _Crafted(name))
        self.pair = Pair(self.cases[0].geo, self.cases[1].geo)
        self.geo = self.cases[0].geo

    def offer(self, slot, g, y, x, cost):
        self.cases[slot].offer(g, y, x, cost)

    def own(self):
        return [c.candidates() for c in self.cases]

    def cands(self):
        return self.pair.cands(self.own())

    def upload(self):
        return [_Synth(self.geo.name, 1).upload(c.lat, c.dd, c.db) for c in self.cases]
