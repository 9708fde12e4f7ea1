"""Helpers of tests/test_rdoq_follow.py: DESIGN.md section 4.17 restated in numpy - the windows of a dependent's samples into its
reference, the reach table of a follow, the flow box of a latent, the claim sets, the component-wide keys and the rounds of a
step over claim sets - and the seeded flows, components and offers the tests run on.

A candidate of a handle is (key, slot, g, y, x, s); its key carries the component-wide uid."""
import numpy as np

from rdoq_joint_ref import geo  # noqa: F401  (_geo with the video fixtures registered)
from test_dependent_deltas import _axes, _regions, _tap_interval  # noqa: F401  (_tap_interval: the tests compare windows() with it)
from test_rdoq import SENTINEL, _reference_step, _Synth
from test_rdoq_rounds import ONES, _as_ref

CELL = 8
EMPTY_BOX = (0xFFFF, 0xFFFF, 0, 0)


# ---- windows ---------------------------------------------------------------------------------------------------------------------
def _axis_interval(taps, f, i, n, g):
    """tests/test_dependent_deltas.py::_tap_interval over arrays: f float32 flows, i the sample index along the axis (broadcast)."""
    f = f.astype(np.float32)
    i = np.broadcast_to(i, f.shape).astype(np.int64)
    if taps >= 6:
        first = i - taps // 2 + 1 + np.clip(np.floor(f), -(n + 16), n + 16).astype(np.int64)
    else:
        s = np.float32((n - 1.0) / 2.0)
        if n == 1:
            lin = np.full(f.shape, -1.0, np.float32)
        else:
            step = np.float32(2.0) / np.float32(n - 1)
            lin = np.where(i < n // 2, np.float64(step) * i - 1.0, -np.float64(step) * (n - 1 - i) + 1.0).astype(np.float32)  # one rounding: an fma
        c = ((lin + (f / s).astype(np.float32)).astype(np.float32) + np.float32(1.0)).astype(np.float32) * s
        c = c.astype(np.float32)
        if taps == 2:
            first = np.floor(np.clip(c, np.float32(0.0), np.float32(n - 1))).astype(np.int64)
        else:
            first = np.clip(np.floor(c), -4.0, n + 4.0).astype(np.int64) - 1

    def index(t):
        return np.clip(np.clip(t, 0, n - 1) + g, 0, n - 1)

    return index(first), index(first + taps - 1)


def windows(motion, which, taps, gflow):
    """int64 [H][W][4]: ya, yb, xa, xb of the window of every sample of the dependent into its reference `which`."""
    H, W = motion.shape[1:]
    ya, yb = _axis_interval(taps, motion[2 * which + 1], np.arange(H)[:, None], H, int(gflow[2 * which + 1]))
    xa, xb = _axis_interval(taps, motion[2 * which], np.arange(W)[None, :], W, int(gflow[2 * which]))
    return np.stack([ya, yb, xa, xb], axis=-1)


# ---- reach table, flow boxes -----------------------------------------------------------------------------------------------------
def reach_table(win, cells_h, cells_w):
    """int64 [cells_h][cells_w][4] = top, left, bottom, right in cells of the dependent; -1 everywhere: nobody reads the cell."""
    H, W = win.shape[:2]
    reach = np.full((cells_h, cells_w, 4), -1, np.int64)
    for Y in range(cells_h):
        for X in range(cells_w):
            w = win[Y * CELL:min((Y + 1) * CELL, H), X * CELL:min((X + 1) * CELL, W)]  # clipped at the ragged border
            t, b = int(w[..., 0].min()) // CELL, int(w[..., 1].max()) // CELL
            l, r = int(w[..., 2].min()) // CELL, int(w[..., 3].max()) // CELL
            part = reach[t:b + 1, l:r + 1]
            new = part[..., 0] < 0
            part[..., 0] = np.where(new, Y, np.minimum(part[..., 0], Y))
            part[..., 1] = np.where(new, X, np.minimum(part[..., 1], X))
            part[..., 2] = np.where(new, Y, np.maximum(part[..., 2], Y))
            part[..., 3] = np.where(new, X, np.maximum(part[..., 3], X))
    return reach


def reach_from_device(words):
    """The device's uint32 {top, left, ~bottom, ~right} as reach_table() states a table."""
    w = words.astype(np.int64)
    out = np.stack([w[..., 0], w[..., 1], 0xFFFFFFFF - w[..., 2], 0xFFFFFFFF - w[..., 3]], axis=-1)
    empty = (w == 0xFFFFFFFF).all(axis=-1)
    assert ((w[..., 0] == 0xFFFFFFFF) == empty).all()  # a word is all ones only when all four are
    out[empty] = -1
    return out


def flow_boxes(reach, boxes):
    """boxes: int32 [h][w][4] influence boxes of a grid.  int64 [h][w][4] flow boxes, EMPTY_BOX where all cells are empty."""
    h, w = boxes.shape[:2]
    out = np.empty((h, w, 4), np.int64)
    big = np.int64(1 << 40)
    lo = np.where(reach[..., :2] < 0, big, reach[..., :2])
    for y in range(h):
        for x in range(w):
            t, l, b, r = boxes[y, x]
            top = lo[t:b + 1, l:r + 1, 0].min()
            if top == big:
                out[y, x] = EMPTY_BOX
            else:
                part = reach[t:b + 1, l:r + 1]
                out[y, x] = (top, lo[t:b + 1, l:r + 1, 1].min(), part[..., 2].max(), part[..., 3].max())
    return out


# ---- E(p), footprints --------------------------------------------------------------------------------------------------------------
def change_region(g_, m, y, x):
    """E(p) of csrc/ccd_lattice.hpp: the clipped footprint from ccd_latent_footprint, widened to even alignment for 4:2:0;
    (top, left, bottom, right) in samples, None for a hyperlatent grid."""
    if g_.hyper[m]:
        return None
    ay, ax = _axes(g_.arch, m)
    even = 1 if g_.fdt == 1 else 0
    (ta, tb), (la, lb) = _regions(ay, even), _regions(ax, even)
    return int(ta[y]), int(la[x]), int(tb[y]), int(lb[x])


# ---- a handle of slots: components, keys, claim sets -----------------------------------------------------------------------------
class Handle:
    """geos: the _Geo of every slot; links: {follower: leader}; follows: [(slot, target, reach table)] in the order they were
    registered.  All slots of a component have congruent rasters."""

    def __init__(self, geos, links=None, follows=()):
        self.geos, self.links, self.follows = list(geos), dict(links or {}), list(follows)
        n = len(self.geos)
        self.leader = [self.links.get(k, k) for k in range(n)]  # the slot whose raster slot k claims its own box in
        comp = list(range(n))

        def find(k):
            while comp[k] != k:
                k = comp[k]
            return k

        def join(a, b):
            a, b = find(a), find(b)
            comp[max(a, b)] = min(a, b)

        for f, l in self.links.items():
            join(f, l)
        for s, t, _ in self.follows:
            join(s, t)
        self.comp = [find(k) for k in range(n)]
        self.offset = [0] * n
        follower_of = {l: f for f, l in self.links.items()}
        nxt = {}
        for k in range(n):  # groups in ascending order of their leader's slot; the leader's latents first
            if k in self.links:
                continue
            at = nxt.get(self.comp[k], 0)
            self.offset[k] = at
            at += sum(self.geos[k].sizes)
            if k in follower_of:
                self.offset[follower_of[k]] = at
                at += sum(self.geos[follower_of[k]].sizes)
            assert at < 2 ** 32
            nxt[self.comp[k]] = at
        self._fbox = {}

    def set_reach(self, slot, k, reach):
        """Replace the reach table of follow k of `slot` (flows rewritten in place)."""
        idx = [i for i, f in enumerate(self.follows) if f[0] == slot][k]
        self.follows[idx] = (slot, self.follows[idx][1], reach)
        self._fbox = {}

    def flow_box(self, slot, k, g):
        """int64 [h][w][4] of follow k of the slot (its k-th in registration order)."""
        if (slot, k, g) not in self._fbox:
            reach = [f for f in self.follows if f[0] == slot][k][2]
            self._fbox[slot, k, g] = flow_boxes(reach, self.geos[slot].boxes()[g])
        return self._fbox[slot, k, g]

    def claim(self, c):
        """[(raster = a leader's slot, rows, columns)]: the own box, then the flow box in the raster of every follow's target."""
        _, slot, g, y, x, _ = c
        t, l, b, r = self.geos[slot].boxes()[g][y, x]
        out = [(self.leader[slot], slice(t, b + 1), slice(l, r + 1))]
        for k, f in enumerate(f for f in self.follows if f[0] == slot):
            t, l, b, r = self.flow_box(slot, k, g)[y, x]
            if t <= b:
                out.append((self.leader[f[1]], slice(int(t), int(b) + 1), slice(int(l), int(r) + 1)))
        return out

    def cands(self, per_slot):
        """per_slot[k]: [(key, g, y, x, s)] as _reference_step lists a slot's own candidates."""
        return [(key + self.offset[k], k, g, y, x, s) for k in range(len(self.geos)) for key, g, y, x, s in per_slot[k]]

    def rasters(self, fill, dtype):
        return {k: np.full((g_.cells_h, g_.cells_w), fill, dtype) for k, g_ in enumerate(self.geos) if self.leader[k] == k}


class Rounds:
    """`max_rounds` rounds over the candidates of a handle.  per_round: the winners of each round; n_open[k]: the candidates of
    slot k that took part in the last round without being selected; blocked: the candidates blocked in a round >= 2."""

    def __init__(self, handle, cands, max_rounds):
        taken = handle.rasters(False, bool)
        claims = {c[:2]: handle.claim(c) for c in cands}
        open_, self.per_round, self.blocked = list(cands), [], []

        def any_taken(c):
            return any(taken[k][rs, cs].any() for k, rs, cs in claims[c[:2]])

        for _ in range(max_rounds):
            if not open_:
                self.per_round.append([])
                continue
            self.blocked += [c for c in open_ if any_taken(c)]                     # 1. blocked for good
            open_ = [c for c in open_ if not any_taken(c)]
            raster = handle.rasters(ONES, np.uint64)
            for c in open_:                                                        # 2. claim
                for k, rs, cs in claims[c[:2]]:
                    np.minimum(raster[k][rs, cs], np.uint64(c[0]), out=raster[k][rs, cs])
            won = [c for c in open_ if all((raster[k][rs, cs] == np.uint64(c[0])).all() for k, rs, cs in claims[c[:2]])]  # 3. select
            for c in won:                                                          # 4. their cells are taken
                for k, rs, cs in claims[c[:2]]:
                    taken[k][rs, cs] = True
            won_keys = {c[:2] for c in won}
            open_ = [c for c in open_ if c[:2] not in won_keys]
            self.per_round.append(won)
        self.n_open = tuple(sum(1 for c in open_ if c[1] == k) for k in range(len(handle.geos)))
        self.selected = [c for won in self.per_round for c in won]


LANE_CELLS = 32  # ccd_rdoq_lane_cells(): an own box of more cells is walked by a wave, the lanes over its cells
DECISIONS = ("blocked, own box", "blocked, flow box only", "lost, own box", "lost, flow box only", "selected")


def decisions(handle, cands, max_rounds):
    """What the rounds of Rounds decide, by the route the device takes to it: {(wave, what): [candidates]} with `wave` whether
    the own box has more than LANE_CELLS cells and `what` of DECISIONS - blocked by a taken cell of the own box, or of a flow box
    alone; lost a select through a cell of the own box, or of a flow box alone (once per round lost); selected."""
    taken = handle.rasters(False, bool)
    claims = {c[:2]: handle.claim(c) for c in cands}
    open_, out = list(cands), {}

    def note(c, what):
        _, rs, cs = claims[c[:2]][0]
        out.setdefault(((rs.stop - rs.start) * (cs.stop - cs.start) > LANE_CELLS, what), []).append(c)

    for _ in range(max_rounds):
        hit = {c[:2]: [bool(taken[k][rs, cs].any()) for k, rs, cs in claims[c[:2]]] for c in open_}
        for c in open_:
            if any(hit[c[:2]]):
                note(c, DECISIONS[0] if hit[c[:2]][0] else DECISIONS[1])
        open_ = [c for c in open_ if not any(hit[c[:2]])]
        raster = handle.rasters(ONES, np.uint64)
        for c in open_:
            for k, rs, cs in claims[c[:2]]:
                np.minimum(raster[k][rs, cs], np.uint64(c[0]), out=raster[k][rs, cs])
        still = []
        for c in open_:
            mine = [bool((raster[k][rs, cs] == np.uint64(c[0])).all()) for k, rs, cs in claims[c[:2]]]
            note(c, DECISIONS[4] if all(mine) else DECISIONS[3] if mine[0] else DECISIONS[2])
            if all(mine):
                for k, rs, cs in claims[c[:2]]:
                    taken[k][rs, cs] = True
            else:
                still.append(c)
        open_ = still
    assert sorted(out.get((False, DECISIONS[4]), []) + out.get((True, DECISIONS[4]), [])) == sorted(Rounds(handle, cands, max_rounds).selected)
    return out


def greedy(handle, cands):
    """The walk over the candidates of every component in ascending key order: a candidate is taken unless its claim set holds a
    taken cell.  (Components do not share a raster, so one walk over (component, key) serves them all.)"""
    taken = handle.rasters(False, bool)
    out = []
    for c in sorted(cands, key=lambda c: (handle.comp[c[1]], c[0])):
        cl = handle.claim(c)
        if not any(taken[k][rs, cs].any() for k, rs, cs in cl):
            for k, rs, cs in cl:
                taken[k][rs, cs] = True
            out.append(c)
    return out


def claim_sets_meet(handle, a, b):
    ra, rb = handle.rasters(False, bool), handle.rasters(False, bool)
    for k, rs, cs in handle.claim(a):
        ra[k][rs, cs] = True
    for k, rs, cs in handle.claim(b):
        rb[k][rs, cs] = True
    return any((ra[k] & rb[k]).any() for k in ra)


def slot_ref(handle, k, lat, slot_cands, per_round):
    """The tests/test_rdoq.py::_Ref of slot k of a step that selected `per_round`."""
    return _as_ref(handle.geos[k], lat, slot_cands, [[(key - handle.offset[k], g, y, x, s) for key, slot, g, y, x, s in won if slot == k]
                                                     for won in per_round])


# ---- seeded flows and maps -------------------------------------------------------------------------------------------------------
def flows(g_, n_refs, seed, amplitude=20.0):
    """float32 [2 n_refs][H][W] uniform in +-amplitude, and a global flow."""
    rng = np.random.default_rng([seed, g_.H, g_.W, 417])
    motion = rng.uniform(-amplitude, amplitude, size=(2 * n_refs, g_.H, g_.W)).astype(np.float32)
    gflow = [int(v) for v in rng.integers(-3, 4, size=4)]
    return motion, gflow


def dep_maps(syn, seed):
    """Seeded dependent maps of a _Synth: int64 [2][h][w] per grid, a few sentinels (conflicts) of their own."""
    rng = np.random.default_rng([seed, len(syn.geo.name), 418])
    out = []
    for hw in syn.geo.hw:
        d = rng.integers(-3000, 3001, size=(2,) + hw, dtype=np.int64)
        d[rng.random(size=d.shape) < 0.02] = SENTINEL
        out.append(d)
    return out


def priced(dd, dep):
    """The distortion map a step with dependent maps prices by: own + dep, the sentinel where either holds it."""
    return [a if b is None else np.where((a == SENTINEL) | (b == SENTINEL), SENTINEL, a + b) for a, b in zip(dd, dep)]


def own_cands(syn, dep=None, mask=None, min_gain=0.0, lat=None, dd=None, db=None, kD=None, kR=None):
    dd = syn.dd if dd is None else dd
    dd = dd if dep is None else priced(dd, dep)
    return _reference_step(syn.geo, syn.lat if lat is None else lat, dd, syn.db if db is None else db, syn.kD if kD is None else kD,
                           syn.kR if kR is None else kR, min_gain, (1 << syn.geo.n) - 1 if mask is None else mask).cands


def synth(name, seed):
    geo(name)
    return _Synth(name, seed)
