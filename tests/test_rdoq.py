"""RDOQ step (ccd_rdoq_*, RdoqStep, RdEvaluator.descend): from the distortion and the rate delta maps, moves
of single latents by +-1 that provably do not interact are chosen on the device and applied in place.

CPU: the geometry.  The influence boxes of ccd_rdoq_influence_box are compared with the contract restated here (area of a pixel,
rate set from the context template exactly as test_rate_deltas.py derives it, footprint from ccd_latent_footprint), and the
superset property is checked by brute force: boxes without a common cell imply disjoint rate sets and disjoint footprints.
GPU, synthetic maps: the six steps of the selection rule restated in numpy, compared exactly.
GPU, end to end: after a step the evaluated SSE has moved by d_sse as integers and the evaluated bits by d_bits within the rate
deltas' own bound."""
import ctypes as C
import math
import os
from typing import NamedTuple

import numpy as np
import pytest

from conftest import ROOT, load_golden

ERR_VALUE, ERR_ARG = -2, -7
SENTINEL = -2 ** 63
TERM_TOL = 24.0 * 2.0 ** -48
ENTRY_POINTS = ["ccd_rdoq_cell", "ccd_rdoq_influence_box", "ccd_rdoq_create", "ccd_rdoq_destroy", "ccd_rdoq_add", "ccd_rdoq_set_maps",
                "ccd_rdoq_step", "ccd_rdoq_wait", "ccd_rdoq_slot_result", "ccd_rdoq_slot_moves"]
GEOMETRY = ["odd18x65", "yuv420_8b", "bicubic190"]
SYNTHETIC = ["odd18x65", "rgb192", "yuv420_8b", "bicubic190"]
# arm.py:501-509: priority of each of the 40 causal positions of the 9 x 9 mask, row-major; the k-th context is the position of rank k
PRIORITY = [38, 35, 30, 25, 23, 31, 36, 37, 39, 33, 28, 21, 20, 6, 15, 22, 29, 34, 32, 18,
            12, 10, 5, 9, 14, 19, 27, 24, 13, 8, 2, 1, 3, 11, 17, 26, 16, 7, 4, 0]


# architectures derived from rgb192 (tests/arm_layouts.py): (spatial contexts, IFCE features), (H, W), ifce_resolution (None: the
# donor's (0, 2)) - 1 .. 40 contexts with 0 .. 31 features at two odd sizes, and IFCE on the coarse grids / on one level's pair
DERIVED = {f"s{sp}_i{fe}_{h}x{w}": ((sp, fe), (h, w), None) for sp, fe in ((1, 0), (24, 7), (40, 31), (40, 0)) for h, w in ((37, 100), (65, 18))}
DERIVED.update({"s6_i3_37x100_ifce3_15": ((6, 3), (37, 100), (3, 15)), "s9_i7_65x18_ifce4_4": ((9, 7), (65, 18), (4, 4))})


def _arch(name):
    """(arch with derived geometry, NN payload, bitdepth, frame_data_type, latent payload, header bytes) of an image fixture or
    of a derived architecture of DERIVED."""
    from cool_chic_amd import writer
    from oracle import oracle_py

    if name in DERIVED:
        import arm_layouts

        (n_sp, n_if), size, res = DERIVED[name]
        stream, _, _ = arm_layouts.build_stream(*arm_layouts.donor(), n_sp + n_if, 1, n_if, seed=len(name), img_size=size, ifce_resolution=res)
    else:
        stream = load_golden(name)[0]
    _, frames = oracle_py.split_stream(stream)
    (fh, ccs), = frames
    hdr, nn, payload = ccs[0]
    return writer.parse_cc_header(hdr), nn, fh.bitdepth, fh.frame_data_type, payload, hdr


class _Geo:
    """The contract of DESIGN.md 4.14 restated from the architecture: rate sets (test_rate_deltas.py::_Case), footprints, areas."""

    def __init__(self, name):
        from cool_chic_amd import rdoq
        from cool_chic_amd.dsens import latent_footprint

        self.name = name
        self.arch, self.nn, self.bd, self.fdt, self.payload, self.hdr = _arch(name)
        a = self.arch
        self.n = a.n_grids
        self.hw = [(int(a.grid_h[g]), int(a.grid_w[g])) for g in range(self.n)]
        self.sizes = [h * w for h, w in self.hw]
        self.first = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.level = [0] * self.n
        for g in range(1, self.n):
            self.level[g] = self.level[g - 1] + (self.hw[g] != self.hw[g - 1])
        self.ifce_in = [int(a.input_features_ifce[g]) for g in range(self.n)]
        self.n_sp = int(a.spatial_context_arm)
        self.taps = [None] * self.n_sp  # (dy, dx): context k of (y, x) is the latent at (y - dy, x + dx)
        for pos, rank in enumerate(PRIORITY):
            if rank < self.n_sp:
                self.taps[rank] = (4 - pos // 9, pos % 9 - 4)
        self.H, self.W = int(a.img_size[0]), int(a.img_size[1])
        self.cell = rdoq.cell()
        self.cells_h, self.cells_w = -(-self.H // self.cell), -(-self.W // self.cell)
        self.hyper = [bool(a.is_hyperlatent[g]) for g in range(self.n)]
        self.foot_box = [None if self.hyper[g] else latent_footprint(a, g) for g in range(self.n)]
        self.lat_grids = [g for g in range(self.n) if not self.hyper[g]]
        self._boxes = None

    # -- the rate set: rectangles (grid, r0, r1, c0, c1), inclusive
    def spatial_dependents(self, m, y, x):
        h, w = self.hw[m]
        out = [(y + dy, x - dx) for dy, dx in self.taps]
        return [(qy, qx) for qy, qx in out if 0 <= qy < h and 0 <= qx < w]

    def ifce_blocks(self, m, y, x):
        out = []
        for g in range(m):
            if self.ifce_in[g] > 0 and g != self.n - 1 and m - g - 1 < self.ifce_in[g]:
                side = 2 << (self.level[m] - self.level[g + 1])
                h, w = self.hw[g]
                r1, c1 = min((y + 1) * side, h) - 1, min((x + 1) * side, w) - 1
                if y * side <= r1 and x * side <= c1:
                    out.append((g, y * side, r1, x * side, c1))
        return out

    def rateset(self, m, y, x):
        return [(m, y, y, x, x)] + [(m, qy, qy, qx, qx) for qy, qx in self.spatial_dependents(m, y, x)] + self.ifce_blocks(m, y, x)

    def n_dep(self, m, y, x):
        return len(self.spatial_dependents(m, y, x)) + sum((r1 - r0 + 1) * (c1 - c0 + 1) for _, r0, r1, c0, c1 in self.ifce_blocks(m, y, x))

    # -- the footprint: clipped luma rectangle (ccd.h: anchored at floor(i * pitch * img / dense)), None for a hyperlatent grid
    def foot(self, m, y, x):
        if self.hyper[m]:
            return None
        a, box = self.arch, self.foot_box[m]
        pitch = 1 << self.lat_grids.index(m)
        g0 = self.lat_grids[0]
        sy, sx = (y * pitch * self.H) // a.grid_h[g0], (x * pitch * self.W) // a.grid_w[g0]
        r = (max(sy + box[0], 0), max(sx + box[1], 0), min(sy + box[2], self.H - 1), min(sx + box[3], self.W - 1))
        return r if r[0] <= r[2] and r[1] <= r[3] else None

    def area(self, g, qy0, qy1, qx0, qx1):
        h0, w0 = self.hw[0]
        lv = self.level[g]
        top, left = ((qy0 << lv) * self.H) // h0, ((qx0 << lv) * self.W) // w0
        bottom = -(-(min((qy1 + 1) << lv, h0) * self.H) // h0) - 1
        right = -(-(min((qx1 + 1) << lv, w0) * self.W) // w0) - 1
        assert 0 <= top <= bottom < self.H and 0 <= left <= right < self.W  # never empty, inside the picture
        return top, left, bottom, right

    def contract_box(self, m, y, x):
        """The influence box in cells as the issue states it."""
        rects = [self.area(*r) for r in self.rateset(m, y, x)]
        f = self.foot(m, y, x)
        if f is not None:
            rects.append(f)
            if self.fdt == 1:  # the halved chroma box, in luma samples
                rects.append(((f[0] >> 1) * 2, (f[1] >> 1) * 2, min((f[2] >> 1) * 2 + 1, self.H - 1), min((f[3] >> 1) * 2 + 1, self.W - 1)))
        top, left = min(r[0] for r in rects), min(r[1] for r in rects)
        bottom, right = max(r[2] for r in rects), max(r[3] for r in rects)
        return top // self.cell, left // self.cell, bottom // self.cell, right // self.cell

    def boxes(self):
        """int32 [h][w][4] per grid through the ABI, once."""
        if self._boxes is None:
            from cool_chic_amd._lib import lib

            L, out = lib(), []
            cells = (C.c_int32 * 4)()
            for g, (h, w) in enumerate(self.hw):
                b = np.zeros((h, w, 4), np.int32)
                for y in range(h):
                    for x in range(w):
                        assert L.ccd_rdoq_influence_box(C.byref(self.arch), self.fdt, g, y, x, cells) == 0
                        b[y, x] = cells[:]
                out.append(b)
            self._boxes = out
        return self._boxes


_GEO = {}


def _geo(name):
    if name not in _GEO:
        _GEO[name] = _Geo(name)
    return _GEO[name]


def _rects_meet(a, b):
    return a[0] <= b[2] and b[0] <= a[2] and a[1] <= b[3] and b[1] <= a[3]


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

    assert cool_chic_amd.RdoqStep.__name__ == "RdoqStep"
    assert all(hasattr(cool_chic_amd.RdoqStep, m) for m in ("add", "set_maps", "step", "wait", "result", "moves", "influence_box"))
    assert hasattr(rd.RdEvaluator, "descend") and rd.StepReport._fields == ("before", "step")


def test_argument_errors_without_a_device():
    from cool_chic_amd._lib import RdoqResult, lib

    L = lib()
    arch = _geo("odd18x65").arch
    assert L.ccd_rdoq_create(0, None) == ERR_ARG
    handle = C.create_string_buffer(512)  # stands for a handle: the calls must return before they look at it
    r = C.cast(handle, C.c_void_p)
    grid = np.zeros(65 * 18, np.int8)
    lat = (C.c_void_p * arch.n_grids)(*[grid.ctypes.data] * arch.n_grids)
    assert L.ccd_rdoq_add(None, C.byref(arch), 0, lat) == ERR_ARG
    assert L.ccd_rdoq_add(r, None, 0, lat) == ERR_ARG
    assert L.ccd_rdoq_add(r, C.byref(arch), 0, None) == ERR_ARG
    for fdt in (-1, 3):
        assert L.ccd_rdoq_add(r, C.byref(arch), fdt, lat) == ERR_ARG
    assert L.ccd_rdoq_set_maps(None, 0, lat, lat) == ERR_ARG
    assert L.ccd_rdoq_set_maps(r, 0, None, lat) == ERR_ARG and L.ccd_rdoq_set_maps(r, 0, lat, None) == ERR_ARG
    assert L.ccd_rdoq_set_maps(r, -1, lat, lat) == ERR_ARG
    one, mask = (C.c_double * 1)(1.0), (C.c_uint64 * 1)(1)
    assert L.ccd_rdoq_step(None, one, one, one, mask, None) == ERR_ARG
    for args in ((None, one, one, mask), (one, None, one, mask), (one, one, None, mask), (one, one, one, None)):
        assert L.ccd_rdoq_step(r, *args, None) == ERR_ARG
    assert L.ccd_rdoq_wait(None, None) == ERR_ARG
    res, dev = RdoqResult(), C.c_void_p()
    assert L.ccd_rdoq_slot_result(None, 0, C.byref(res)) == ERR_ARG and L.ccd_rdoq_slot_result(r, 0, None) == ERR_ARG
    assert L.ccd_rdoq_slot_result(r, -1, C.byref(res)) == ERR_ARG
    assert L.ccd_rdoq_slot_moves(None, 0, 0, C.byref(dev)) == ERR_ARG and L.ccd_rdoq_slot_moves(r, 0, 0, None) == ERR_ARG
    assert L.ccd_rdoq_slot_moves(r, -1, 0, C.byref(dev)) == ERR_ARG and L.ccd_rdoq_slot_moves(r, 0, -1, C.byref(dev)) == ERR_ARG
    assert not dev.value and bytes(handle) == bytes(512)
    cells = (C.c_int32 * 4)()
    assert L.ccd_rdoq_influence_box(None, 0, 0, 0, 0, cells) == ERR_ARG and L.ccd_rdoq_influence_box(C.byref(arch), 0, 0, 0, 0, None) == ERR_ARG
    assert L.ccd_rdoq_influence_box(C.byref(arch), 3, 0, 0, 0, cells) == ERR_ARG
    for g, y, x in ((-1, 0, 0), (arch.n_grids, 0, 0), (0, -1, 0), (0, arch.grid_h[0], 0), (0, 0, arch.grid_w[0])):
        assert L.ccd_rdoq_influence_box(C.byref(arch), 0, g, y, x, cells) == ERR_ARG
    L.ccd_rdoq_destroy(None)


def test_cell_size():
    from cool_chic_amd import rdoq

    assert rdoq.cell() >= 2 and rdoq.cell() % 2 == 0


def _pairs(geo, g1, g2, rng):
    """[(p, q)] of grids g1, g2: every pair when there are at most 4 096, else 2 000 seeded ones; and, for seeded p, latents q whose
    box does not meet p's but would if it were one cell larger on every side."""
    boxes = geo.boxes()
    (h1, w1), (h2, w2) = geo.hw[g1], geo.hw[g2]
    n1, n2 = h1 * w1, h2 * w2
    if n1 * n2 <= 4096:
        pairs = [(i, j) for i in range(n1) for j in range(n2) if g1 != g2 or i < j]
    else:
        pairs = list(zip(rng.integers(n1, size=2000).tolist(), rng.integers(n2, size=2000).tolist()))
    b2 = boxes[g2].reshape(-1, 4)
    for i in rng.integers(n1, size=24).tolist():
        t, l, b, r = boxes[g1].reshape(-1, 4)[i]
        meets = (b2[:, 0] <= b) & (t <= b2[:, 2]) & (b2[:, 1] <= r) & (l <= b2[:, 3])
        near = (b2[:, 0] <= b + 1) & (t - 1 <= b2[:, 2]) & (b2[:, 1] <= r + 1) & (l - 1 <= b2[:, 3])
        adjacent = np.nonzero(near & ~meets)[0]
        if len(adjacent):
            pairs += [(i, int(j)) for j in rng.choice(adjacent, size=min(8, len(adjacent)), replace=False)]
    return [(divmod(i, w1), divmod(j, w2)) for i, j in pairs if g1 != g2 or i != j]


@pytest.mark.parametrize("name", GEOMETRY + list(DERIVED))
def test_boxes_without_a_common_cell_are_independent(name):
    geo = _geo(name)
    boxes = geo.boxes()
    rng = np.random.default_rng(2024)
    sh = 1 if geo.fdt == 1 else 0
    n_disjoint = n_meeting = n_adjacent = 0
    rs_cache, ft_cache = {}, {}
    for g1 in range(geo.n):
        for g2 in range(g1, geo.n):
            for (y1, x1), (y2, x2) in _pairs(geo, g1, g2, rng):
                a, b = boxes[g1][y1, x1], boxes[g2][y2, x2]
                if _rects_meet(a, b):
                    n_meeting += 1
                    continue
                n_disjoint += 1
                n_adjacent += _rects_meet((a[0] - 1, a[1] - 1, a[2] + 1, a[3] + 1), b)
                p, q = (g1, y1, x1), (g2, y2, x2)
                for k in (p, q):
                    if k not in rs_cache:
                        rs_cache[k], ft_cache[k] = geo.rateset(*k), geo.foot(*k)
                shared = [(r, s) for r in rs_cache[p] for s in rs_cache[q]
                          if r[0] == s[0] and r[1] <= s[2] and s[1] <= r[2] and r[3] <= s[4] and s[3] <= r[4]]
                assert not shared, (name, p, q, shared[:2])
                fp, fq = ft_cache[p], ft_cache[q]
                if fp is not None and fq is not None:
                    assert not _rects_meet(fp, fq), (name, p, q, fp, fq)
                    if sh:  # chroma planes: floor(H / 2) x floor(W / 2), the box halved and rounded outwards
                        cp = (fp[0] >> 1, fp[1] >> 1, fp[2] >> 1, fp[3] >> 1)
                        cq = (fq[0] >> 1, fq[1] >> 1, fq[2] >> 1, fq[3] >> 1)
                        assert not _rects_meet(cp, cq), (name, p, q, cp, cq)
    print(f"{name}: {n_disjoint} pairs without a common cell ({n_adjacent} of them adjacent), {n_meeting} with one")
    assert n_disjoint >= 1 and n_meeting >= 1 and n_adjacent >= 1


@pytest.mark.parametrize("name", GEOMETRY + list(DERIVED))
def test_boxes_are_the_contract_clipped_not_shifted(name):
    geo = _geo(name)
    boxes = geo.boxes()
    rng = np.random.default_rng(5)
    n_hyper = 0
    for g, (h, w) in enumerate(geo.hw):
        b = boxes[g]
        assert (b[..., 0] >= 0).all() and (b[..., 1] >= 0).all() and (b[..., 2] < geo.cells_h).all() and (b[..., 3] < geo.cells_w).all()
        assert (b[..., 0] <= b[..., 2]).all() and (b[..., 1] <= b[..., 3]).all()
        # monotone in the position: a box never moves backwards
        assert (np.diff(b[..., 0], axis=0) >= 0).all() and (np.diff(b[..., 2], axis=0) >= 0).all()
        assert (np.diff(b[..., 1], axis=1) >= 0).all() and (np.diff(b[..., 3], axis=1) >= 0).all()
        where = {(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2)}
        if geo.hyper[g] or h * w <= 64:
            where |= {(y, x) for y in range(h) for x in range(w)}
        else:
            where |= {(int(rng.integers(h)), int(rng.integers(w))) for _ in range(40)}
        for y, x in sorted(where):
            assert tuple(b[y, x]) == geo.contract_box(g, y, x), (name, g, y, x)
        n_hyper += geo.hyper[g]
        # clipped, not shifted: a box holds the cells of its own pixel's area wherever the latent lies, and the corner boxes
        # reach the raster's edges (the equality with contract_box above is the exact statement: it clips with max / min)
        for y, x in sorted(where):
            t, l, bt, r = geo.area(g, y, y, x, x)
            assert b[y, x][0] <= t // geo.cell and b[y, x][1] <= l // geo.cell and b[y, x][2] >= bt // geo.cell and b[y, x][3] >= r // geo.cell
        assert b[0, 0][0] == 0 and b[0, 0][1] == 0 and b[h - 1, w - 1][2] == geo.cells_h - 1 and b[h - 1, w - 1][3] == geo.cells_w - 1
    if name == "odd18x65":
        assert n_hyper >= 1  # a hyperlatent grid: no footprint, the box is its rate set's (compared with the contract above)


# ---- GPU: synthetic maps ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cool_chic_amd import RdoqStep, _lib

    _lib.lib()
    return RdoqStep


PAD = 64  # guard bytes around every grid of a latent buffer


class _Synth:
    """Seeded latents and maps of one fixture on the host, and their device copies."""

    def __init__(self, name, seed=0):
        self.geo = geo = _geo(name)
        rng = np.random.default_rng([seed, len(name)])
        self.lat, self.dd, self.db = [], [], []
        for g, hw in enumerate(geo.hw):
            lat = rng.integers(-12, 13, size=hw, dtype=np.int8)
            where = rng.choice(lat.size, size=min(lat.size, 6), replace=False)
            lat.flat[where] = rng.choice([-64, 63], size=len(where))
            # most moves cost: the candidates are sparse, so that those of the middle grids can own their boxes too
            dd = rng.integers(-5000 if g < 3 else 5000, 39 * 5000 + 1, size=(2,) + hw, dtype=np.int64)
            db = (rng.standard_normal((2,) + hw) * 3.0).astype(np.float32)
            # every grid offers at least one move that pays, a weak one: a coarse candidate's box is the whole raster, and with a
            # strong key it would leave the step a single move (test_crafted_maps has that case)
            dd[0].flat[0], db[0].flat[0] = -1 - g, -2.0 ** -10
            if lat.flat[0] == -64:
                lat.flat[0] = 0
            dd[0][lat == -64] = SENTINEL
            dd[1][lat == 63] = SENTINEL
            db[0][lat == -64] = np.inf
            db[1][lat == 63] = np.inf
            self.lat.append(lat); self.dd.append(dd); self.db.append(db)
        self.kD, self.kR = 1.0 / 3000.0, 0.25
        self.pos, at = [], 0
        for a in self.lat:
            at = (at + PAD + 255) // 256 * 256 + 3
            self.pos.append(at)
            at += a.size
        self.buf_len = at + PAD

    def host_buffer(self, lat=None):
        host = np.full(self.buf_len, 0x55, np.uint8)
        for p, a in zip(self.pos, self.lat if lat is None else lat):
            host[p:p + a.size] = a.astype(np.int8).view(np.uint8).ravel()
        return host

    def upload(self, lat=None, dd=None, db=None):
        import torch

        self.buf = torch.from_numpy(self.host_buffer(lat).view(np.int8)).cuda()
        self.dd_dev = [torch.from_numpy(a).cuda() for a in (self.dd if dd is None else dd)]
        self.db_dev = [torch.from_numpy(a).cuda() for a in (self.db if db is None else db)]
        torch.cuda.synchronize()
        return self

    def add_to(self, step, dd_null=()):
        slot = step.add(self.geo.arch, self.geo.fdt, [self.buf.data_ptr() + p for p in self.pos], owner=self.buf)
        step.set_maps(slot, [None if g in dd_null else t.data_ptr() for g, t in enumerate(self.dd_dev)], [t.data_ptr() for t in self.db_dev],
                      owner=(self.dd_dev, self.db_dev))
        return slot

    def latents_now(self):
        host = self.buf.cpu().numpy().view(np.uint8)
        return [host[p:p + a.size].view(np.int8).reshape(a.shape).copy() for p, a in zip(self.pos, self.lat)], host


class _Ref(NamedTuple):
    moves: list        # int8 [h][w] per grid
    after: list        # the latents after the step
    n_candidates: int
    chosen: list       # [(g, y, x, s)]
    n_lost: int        # candidates that lost a cell
    cands: list        # [(key, g, y, x, s)]


def _reference_step(geo, lat, dd, db, kD, kR, min_gain, mask):
    """The six steps of the rule in numpy."""
    boxes = geo.boxes()
    cands = []  # (key, g, y, x, s)
    with np.errstate(over="ignore", invalid="ignore"):
        for g, (h, w) in enumerate(geo.hw):
            v = lat[g].astype(np.int64)
            c64, c32, exists = [], [], []
            for k, s in enumerate((-1, 1)):
                d = dd[g][k] if dd[g] is not None else np.zeros((h, w), np.int64)
                exists.append((d != SENTINEL) & np.isfinite(db[g][k]) & (v >= -64) & (v <= 63) & (v + s >= -64) & (v + s <= 63))
                c = d.astype(np.float64) * np.float64(kD) + db[g][k].astype(np.float64) * np.float64(kR)
                c64.append(c); c32.append(c.astype(np.float32))
            k = np.where(exists[0] & exists[1], c32[1] < c32[0], exists[1]).astype(np.int64)
            pick = lambda a: np.where(k == 1, a[1], a[0])  # noqa: E731
            cand = bool((mask >> g) & 1) & pick(exists) & (pick(c64) < -np.float64(min_gain))
            bits = pick(c32).astype(np.float32).view(np.uint32).astype(np.uint64)
            order = bits ^ np.where(bits >> np.uint64(31), np.uint64(0xFFFFFFFF), np.uint64(0x80000000))
            uid = (int(geo.first[g]) + np.arange(h * w, dtype=np.uint64)).reshape(h, w)
            key = (order << np.uint64(32)) | uid
            for y, x in zip(*np.nonzero(cand)):
                cands.append((int(key[y, x]), g, int(y), int(x), int(2 * k[y, x] - 1)))
    raster = np.full((geo.cells_h, geo.cells_w), np.uint64(2 ** 64 - 1), np.uint64)
    for key, g, y, x, s in cands:
        t, l, b, r = boxes[g][y, x]
        np.minimum(raster[t:b + 1, l:r + 1], np.uint64(key), out=raster[t:b + 1, l:r + 1])
    moves = [np.zeros(hw, np.int8) for hw in geo.hw]
    after = [a.copy() for a in lat]
    chosen = []
    for key, g, y, x, s in cands:
        t, l, b, r = boxes[g][y, x]
        if (raster[t:b + 1, l:r + 1] == np.uint64(key)).all():
            moves[g][y, x] = s
            after[g][y, x] += s
            chosen.append((g, y, x, s))
    return _Ref(moves, after, len(cands), chosen, len(cands) - len(chosen), cands)


def _device_outcome(step, slot, syn):
    import torch

    res = step.result(slot)
    moves = [torch.as_tensor(step.moves(slot, g), device="cuda").cpu().numpy().copy() for g in range(syn.geo.n)]
    after, raw = syn.latents_now()
    return res, moves, after, raw


def _compare(syn, outcome, ref, kD, kR, what, dd=None, db=None):
    """dd, db: the host maps the step read (a None entry of dd: zeros); the seeded ones by default."""
    res, moves, after, raw = outcome
    ref_moves, ref_after, n_cand, chosen = ref.moves, ref.after, ref.n_candidates, ref.chosen
    geo = syn.geo
    dd, db = syn.dd if dd is None else dd, syn.db if db is None else db
    for g in range(geo.n):
        assert moves[g].dtype == np.int8 and np.array_equal(moves[g], ref_moves[g]), (what, geo.name, g, int((moves[g] != ref_moves[g]).sum()))
        assert np.array_equal(after[g], ref_after[g]), (what, geo.name, g)
    assert res.n_candidates == n_cand and res.n_moves == len(chosen), (what, geo.name, res, n_cand, len(chosen))
    assert list(res.n_moves_grid) == [int(np.count_nonzero(m)) for m in ref_moves], (what, geo.name)
    sse = sum(int(dd[g][(s + 1) // 2, y, x]) if dd[g] is not None else 0 for g, y, x, s in chosen)
    assert res.d_sse == sse, (what, geo.name, res.d_sse, sse)
    bits = [float(db[g][(s + 1) // 2, y, x]) for g, y, x, s in chosen]
    assert abs(res.d_bits - math.fsum(bits)) <= len(bits) * 2.0 ** -52 * math.fsum(abs(b) for b in bits), (what, geo.name, res.d_bits, math.fsum(bits))
    assert res.d_cost == kD * float(res.d_sse) + kR * res.d_bits
    # write scope: the guard bytes around every grid are what they were
    guard = np.ones(len(raw), bool)
    for p, a in zip(syn.pos, syn.lat):
        guard[p:p + a.size] = False
    assert (raw[guard] == 0x55).all(), (what, geo.name)


def _run(step, kD, kR, min_gain, masks):
    step.step(kD, kR, min_gain, masks)
    step.wait()


def _fresh(names, seed=0):
    return [_Synth(n, seed).upload() for n in names]


@pytest.mark.gpu
def test_four_architectures_in_one_launch(gpu):
    syns = _fresh(SYNTHETIC)
    step = gpu(0)
    for s in syns:
        s.add_to(step)
    full = [(1 << s.geo.n) - 1 for s in syns]
    _run(step, [s.kD for s in syns], [s.kR for s in syns], [0.0] * len(syns), full)
    for slot, s in enumerate(syns):
        ref = _reference_step(s.geo, s.lat, s.dd, s.db, s.kD, s.kR, 0.0, full[slot])
        # the reference keeps the test honest: candidates lose cells, every grid of the mask has a candidate
        assert ref.n_lost >= 1 and len(ref.chosen) >= 2, (s.geo.name, ref.n_candidates, len(ref.chosen))
        assert {c[1] for c in ref.cands} == set(range(s.geo.n)), s.geo.name
        _compare(s, _device_outcome(step, slot, s), ref, s.kD, s.kR, "four in one handle")
        # the maps are only read
        for g in range(s.geo.n):
            assert np.array_equal(s.dd_dev[g].cpu().numpy(), s.dd[g]) and np.array_equal(s.db_dev[g].cpu().numpy().view(np.uint32), s.db[g].view(np.uint32))
        print(f"{s.geo.name}: {ref[2]} candidates, {len(ref[3])} moves, {ref[4]} lost a cell")
    step.close()


def _one(gpu, syn, kD, kR, min_gain, mask, what, dd_null=()):
    step = gpu(0)
    syn.add_to(step, dd_null)
    _run(step, [kD], [kR], [min_gain], [mask])
    dd = [None if g in dd_null else a for g, a in enumerate(syn.dd_now)]
    ref = _reference_step(syn.geo, syn.lat_now, dd, syn.db_now, kD, kR, min_gain, mask)
    _compare(syn, _device_outcome(step, 0, syn), ref, kD, kR, what, dd, syn.db_now)
    step.close()
    return ref


@pytest.mark.gpu
def test_crafted_maps(gpu):
    base = _Synth("odd18x65", 1)
    geo = base.geo
    full = (1 << geo.n) - 1

    def case(lat=None, dd=None, db=None):
        s = _Synth("odd18x65", 1)
        s.lat_now = [a.copy() for a in (base.lat if lat is None else lat)]
        s.dd_now = [a.copy() for a in (base.dd if dd is None else dd)]
        s.db_now = [a.copy() for a in (base.db if db is None else db)]
        return s.upload(s.lat_now, s.dd_now, s.db_now)

    mid = [np.zeros_like(a) for a in base.lat]
    # all costs equal: the position decides
    s = case(mid, [np.full_like(a, -7) for a in base.dd], [np.zeros_like(a) for a in base.db])
    ref = _one(gpu, s, 1.0, 1.0, 0.0, full, "equal costs")
    assert ref[2] == sum(geo.sizes) and all(mv[3] == -1 for mv in ref[3]) and (0, 0, 0, -1) in ref[3]
    # nothing on offer: sentinels and +inf
    s = case(mid, [np.full_like(a, SENTINEL) for a in base.dd], [np.full_like(a, np.inf) for a in base.db])
    ref = _one(gpu, s, 1.0, 1.0, 0.0, full, "sentinels")
    assert ref[2] == 0 and not ref[3]
    s = case(mid, [np.full_like(a, -7) for a in base.dd], [np.full_like(a, np.inf) for a in base.db])
    assert _one(gpu, s, 1.0, 1.0, 0.0, full, "+inf")[2] == 0
    # latents at the alphabet's ends with the sentinel on one sign; and a stale map that offers +1 at a 63
    ends = [np.where(np.arange(a.size).reshape(a.shape) % 2 == 0, -64, 63).astype(np.int8) for a in base.lat]
    dd = [np.full_like(a, -7) for a in base.dd]
    for g in range(geo.n):
        dd[g][0][ends[g] == -64] = SENTINEL
        dd[g][1][ends[g] == 63] = SENTINEL
    s = case(ends, dd, [np.zeros_like(a) for a in base.db])
    ref = _one(gpu, s, 1.0, 1.0, 0.0, full, "alphabet ends")
    assert ref[2] == sum(geo.sizes) and all((s_ == 1) == (ends[g][y, x] == -64) for g, y, x, s_ in ref[3])
    stale = [np.full_like(a, 63) for a in base.lat]
    dd = [np.stack([np.full(hw, SENTINEL, np.int64), np.full(hw, -7, np.int64)]) for hw in geo.hw]
    s = case(stale, dd, [np.zeros_like(a) for a in base.db])
    assert _one(gpu, s, 1.0, 1.0, 0.0, full, "stale +1 at 63")[2] == 0
    # one very negative entry on the coarsest grid, whose box is the whole raster: exactly one move
    last = geo.n - 1
    assert tuple(geo.boxes()[last][0, 0]) == (0, 0, geo.cells_h - 1, geo.cells_w - 1)
    dd = [a.copy() for a in base.dd]
    dd[last][1, 0, 0] = -10 ** 9
    db = [a.copy() for a in base.db]
    db[last][1, 0, 0] = 0.0
    lat = [a.copy() for a in base.lat]
    lat[last][0, 0] = 0
    s = case(lat, dd, db)
    ref = _one(gpu, s, base.kD, base.kR, 0.0, full, "one owner of the raster")
    assert ref[2] > 10 and ref[3] == [(last, 0, 0, 1)]
    # a mask with a single grid; a NULL distortion map for a grid (zeros)
    s = case()
    ref = _one(gpu, s, base.kD, base.kR, 0.0, 1 << 1, "grid 1 alone")
    assert ref[3] and all(mv[0] == 1 for mv in ref[3])
    s = case()
    ref = _one(gpu, s, base.kD, base.kR, 0.0, full, "no distortion map for grid 0", dd_null=(0,))
    assert ref[2] > 0
    # a least gain that leaves the best move only
    s = case()
    all_ref = _reference_step(geo, base.lat, base.dd, base.db, base.kD, base.kR, 0.0, full)
    costs = sorted(float(base.dd[g][(s_ + 1) // 2, y, x]) * base.kD + float(base.db[g][(s_ + 1) // 2, y, x]) * base.kR for _, g, y, x, s_ in all_ref.cands)
    assert len(costs) > 10 and costs[0] < costs[1] < 0
    ref = _one(gpu, s, base.kD, base.kR, -(costs[0] + costs[1]) / 2, full, "least gain")
    assert ref[2] == 1 and len(ref[3]) == 1


def _words(outcome):
    res, moves, after, raw = outcome
    return (res.n_candidates, res.n_moves, res.n_moves_grid, res.d_sse, np.float64(res.d_bits).view(np.uint64).item(),
            np.float64(res.d_cost).view(np.uint64).item(), [m.tobytes() for m in moves], raw.tobytes())


@pytest.mark.gpu
def test_repeatability(gpu):
    import torch

    syns = _fresh(SYNTHETIC)
    step = gpu(0)
    for s in syns:
        s.add_to(step)
    args = ([s.kD for s in syns], [s.kR for s in syns], [0.0] * len(syns), [(1 << s.geo.n) - 1 for s in syns])
    _run(step, *args)
    first = [_words(_device_outcome(step, k, s)) for k, s in enumerate(syns)]
    assert all(w[1] >= 2 for w in first)
    for s in syns:  # the latents as they were
        s.buf.copy_(torch.from_numpy(s.host_buffer().view(np.int8)))
    torch.cuda.synchronize()
    _run(step, *args)
    assert [_words(_device_outcome(step, k, s)) for k, s in enumerate(syns)] == first
    step.close()
    for k, name in enumerate(SYNTHETIC):  # alone
        s, = _fresh([name])
        alone = gpu(0)
        s.add_to(alone)
        _run(alone, [s.kD], [s.kR], [0.0], [(1 << s.geo.n) - 1])
        assert _words(_device_outcome(alone, 0, s)) == first[k], name
        alone.close()


@pytest.mark.gpu
def test_argument_checks_on_a_live_handle(gpu):
    from cool_chic_amd._lib import RdoqResult, lib

    L = lib()
    s, other = _fresh(["odd18x65", "odd18x65"])  # a buffer of its own for each slot: a step writes the latents
    step = gpu(0)
    h = step._h
    one, mask = (C.c_double * 2)(1.0, 1.0), (C.c_uint64 * 2)(1, 1)
    res, dev = RdoqResult(), C.c_void_p()
    assert L.ccd_rdoq_step(h, one, one, one, mask, None) == 0 and L.ccd_rdoq_wait(h, None) == 0  # an empty handle steps nothing
    lat = (C.c_void_p * s.geo.n)(*[s.buf.data_ptr() + p for p in s.pos])
    assert L.ccd_rdoq_add(h, C.byref(s.geo.arch), 0, (C.c_void_p * s.geo.n)()) == ERR_ARG  # a NULL grid
    assert L.ccd_rdoq_add(h, C.byref(s.geo.arch), s.geo.fdt, lat) == 0
    assert L.ccd_rdoq_step(h, one, one, one, mask, None) == ERR_ARG  # no maps yet
    dd = (C.c_void_p * s.geo.n)(*[t.data_ptr() for t in s.dd_dev])
    db = (C.c_void_p * s.geo.n)(*[t.data_ptr() for t in s.db_dev])
    assert L.ccd_rdoq_set_maps(h, 1, dd, db) == ERR_ARG
    assert L.ccd_rdoq_set_maps(h, 0, dd, (C.c_void_p * s.geo.n)()) == ERR_ARG  # a rate map is not optional
    assert L.ccd_rdoq_set_maps(h, 0, dd, db) == 0
    assert L.ccd_rdoq_slot_result(h, 0, C.byref(res)) == ERR_ARG and L.ccd_rdoq_slot_moves(h, 0, 0, C.byref(dev)) == ERR_ARG  # no step yet
    before = s.buf.cpu().numpy().copy()
    for bad in (-1.0, float("nan"), float("inf")):
        for k in range(3):
            args = [(C.c_double * 1)(1.0) for _ in range(3)]
            args[k] = (C.c_double * 1)(bad)
            assert L.ccd_rdoq_step(h, *args, mask, None) == ERR_ARG, (bad, k)
    assert np.array_equal(s.buf.cpu().numpy(), before)
    assert L.ccd_rdoq_step(h, one, one, one, mask, None) == 0
    assert L.ccd_rdoq_step(h, one, one, one, mask, None) == ERR_ARG  # one step in flight
    assert L.ccd_rdoq_slot_result(h, 0, C.byref(res)) == ERR_ARG and L.ccd_rdoq_add(h, C.byref(s.geo.arch), s.geo.fdt, lat) == ERR_ARG
    assert L.ccd_rdoq_wait(h, None) == 0
    assert L.ccd_rdoq_slot_result(h, 0, C.byref(res)) == 0 and res.n_grids == s.geo.n
    assert not any(res.n_moves_grid[g] for g in range(s.geo.n, len(res.n_moves_grid)))  # the entries past the slot's grids are zero
    assert L.ccd_rdoq_slot_moves(h, 0, 0, C.byref(dev)) == s.geo.sizes[0] and dev.value
    for slot, grid in ((1, 0), (0, s.geo.n)):
        assert L.ccd_rdoq_slot_moves(h, slot, grid, C.byref(dev)) == ERR_ARG
    # a slot added after a step is covered by the next one, and the handle steps again
    lat1 = (C.c_void_p * s.geo.n)(*[other.buf.data_ptr() + p for p in other.pos])
    assert L.ccd_rdoq_add(h, C.byref(s.geo.arch), s.geo.fdt, lat1) == 1
    assert L.ccd_rdoq_slot_result(h, 1, C.byref(res)) == ERR_ARG
    assert L.ccd_rdoq_set_maps(h, 1, dd, db) == 0
    assert L.ccd_rdoq_step(h, one, one, one, mask, None) == 0 and L.ccd_rdoq_wait(h, None) == 0
    assert L.ccd_rdoq_slot_result(h, 1, C.byref(res)) == 0
    step.close()


# ---- GPU: end to end --------------------------------------------------------------------------------------------------
FDT_NAMES = ["rgb", "yuv420", "yuv444"]


class _Picture:
    """A fixture's own latents (from the oracle's entropy decode), its source = what they decode to, and a seeded tenth of the
    positions moved by +-1 on a device buffer the evaluator is given."""

    def __init__(self, oracle, name, seed=0):
        import torch

        from cool_chic_amd import DecodeBatch
        from cool_chic_amd.quality import _planes_to_frame_data

        self.geo = geo = _geo(name)
        self.own = [np.ascontiguousarray(a, np.int8) for a in oracle.decode_coolchic(geo.hdr, geo.nn, geo.payload, stop_after_entropy=True)["latent"]]
        dec = DecodeBatch(0)
        dec.add_latents(geo.arch, geo.nn, self.own, geo.bd, geo.fdt)
        dec.run(); dec.wait()
        self.source = _planes_to_frame_data(dec.planes(0), geo.bd, FDT_NAMES[geo.fdt])
        dec.close()
        rng = np.random.default_rng([seed, len(name)])
        self.moved = []
        for a in self.own:
            m = a.astype(np.int64) + np.where(rng.random(a.shape) < 0.1, rng.choice([-1, 1], size=a.shape), 0)
            self.moved.append(np.clip(m, -64, 63).astype(np.int8))
        self.sizes = geo.sizes
        self.off = np.concatenate([[0], np.cumsum([(s + 255) // 256 * 256 for s in self.sizes])]).astype(np.int64)
        self.torch = torch

    def device_latents(self):
        row = np.zeros(int(self.off[-1]), np.int8)
        for g, a in enumerate(self.moved):
            row[self.off[g]:self.off[g] + a.size] = a.ravel()
        return self.torch.from_numpy(row).cuda()

    def ptrs(self, dev):
        return [dev.data_ptr() + int(self.off[g]) for g in range(self.geo.n)]

    def grids(self, dev):
        host = dev.cpu().numpy()
        return [host[self.off[g]:self.off[g] + s].reshape(self.geo.hw[g]).copy() for g, s in enumerate(self.sizes)]


_PICTURES = {}


def _picture(oracle, name):
    if name not in _PICTURES:
        _PICTURES[name] = _Picture(oracle, name)
    return _PICTURES[name]


def _step_bound(ev, slot, pic, n_symbols):
    """The issue's bound on |new total_bits - old - d_bits| for the step that just ran, from its move maps and the rate maps the
    step read: sum over the moves of 2 (1 + |dep(p)|) TERM_TOL + |dBits(p)| 2^-23, plus 2 n_symbols TERM_TOL."""
    import torch

    geo, bound, n = pic.geo, 2.0 * n_symbols * TERM_TOL, 0
    for g in range(geo.n):
        mv = torch.as_tensor(ev.step_moves(slot, g), device="cuda").cpu().numpy()
        db = torch.as_tensor(ev.rate_delta_map(slot, g), device="cuda").cpu().numpy()
        for y, x in zip(*np.nonzero(mv)):
            bound += 2.0 * (1 + geo.n_dep(g, int(y), int(x))) * TERM_TOL + abs(float(db[(int(mv[y, x]) + 1) // 2, y, x])) * 2.0 ** -23
            n += 1
    return bound, n


# The grids that may move in the end-to-end tests.  A candidate of a coarse grid owns the whole raster and, being worth thousands
# of squared-error units, beats everything: with every grid admitted a step of a real picture is one move (measured: rgb192,
# 16 101 candidates, one move on grid 3).  The mask is the user's lever; the tests pull it.
ONE_STEP_GRIDS = {"rgb192": (0, 1), "yuv420_8b": (0, 1), "odd18x65": (0,)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rgb192", "yuv420_8b", "odd18x65"])
def test_one_step_predicts_exactly(gpu, oracle, name):
    from cool_chic_amd import RdEvaluator

    pic = _picture(oracle, name)
    for lmbda in (1e-4, 5e-3):
        dev = pic.device_latents()
        ev = RdEvaluator(0)
        ev.add(pic.geo.arch, pic.geo.nn, pic.ptrs(dev), pic.source, owner=dev)
        (rep,), = ev.descend(lmbda, max_steps=1, grids=ONE_STEP_GRIDS[name])
        before, step = rep.before, rep.step
        bound, n = _step_bound(ev, 0, pic, int(before.rate.n_symbols.sum()))
        assert n == step.n_moves >= 2 and step.n_candidates > step.n_moves, (name, lmbda, step)
        after, = ev.evaluate(lmbda)
        d_sse = sum(after.quality.sse) - sum(before.quality.sse)
        d_bits = after.rate.total_bits - before.rate.total_bits
        print(f"{name} lambda {lmbda}: {step.n_candidates} candidates, {step.n_moves} moves, d_sse {d_sse} (step {step.d_sse}), "
              f"d_bits {d_bits!r} (step {step.d_bits!r}, |diff| {abs(d_bits - step.d_bits):.3g}, bound {bound:.3g}), "
              f"cost {before.cost!r} -> {after.cost!r} (step {step.d_cost!r})")
        assert d_sse == step.d_sse
        assert abs(d_bits - step.d_bits) <= bound
        assert step.d_cost < 0 and after.cost < before.cost
        ev.close()


@pytest.mark.gpu
def test_descent_and_round_trip(gpu, oracle):
    from cool_chic_amd import DecodeBatch, EncodeBatch, RdEvaluator, writer

    names, lmbda = ["odd18x65", "yuv420_8b"], 1e-3
    pics = [_picture(oracle, n) for n in names]

    def evaluator():
        devs = [p.device_latents() for p in pics]
        ev = RdEvaluator(0)
        for p, d in zip(pics, devs):
            ev.add(p.geo.arch, p.geo.nn, p.ptrs(d), p.source, owner=d)
        return ev, devs

    # A: one step at a time, so that every step's bound can be formed from its own maps
    ev, devs = evaluator()
    reports, bounds = [], []
    for _ in range(6):
        rep, = ev.descend(lmbda, max_steps=1, grids=(0, 1, 2))
        reports.append(rep)
        bounds.append([_step_bound(ev, s, p, int(rep[s].before.rate.n_symbols.sum()))[0] for s, p in enumerate(pics)])
        if not any(r.step.n_moves for r in rep):
            break
    final = ev.evaluate(lmbda)
    assert any(r.step.n_moves for r in reports[0])
    for s, p in enumerate(pics):
        costs = [rep[s].before.cost for rep in reports] + [final[s].cost]
        for k, rep in enumerate(reports):
            st = rep[s].step
            if st.n_moves:
                kR = lmbda / float(p.source.n_pixels)
                print(f"{p.geo.name} step {k}: {st.n_candidates} candidates, {st.n_moves} moves, cost {costs[k]!r} -> {costs[k + 1]!r}, "
                      f"d_cost {st.d_cost!r}, |diff| {abs(costs[k + 1] - costs[k] - st.d_cost):.3g}, bound {bounds[k][s] * kR:.3g}")
                assert costs[k + 1] < costs[k]
                assert abs(costs[k + 1] - costs[k] - st.d_cost) <= bounds[k][s] * kR
            else:
                assert costs[k + 1] == costs[k]
        assert costs[-1] < costs[0]
    # B: the same descent in one call gives the same reports and the same latents
    ev_b, devs_b = evaluator()
    reports_b = ev_b.descend(lmbda, max_steps=6, grids=(0, 1, 2))
    assert len(reports_b) == len(reports)
    for ra, rb in zip(reports, reports_b):
        assert [r.step for r in ra] == [r.step for r in rb] and [r.before.cost for r in ra] == [r.before.cost for r in rb]
    for p, da, db in zip(pics, devs, devs_b):
        assert np.array_equal(da.cpu().numpy(), db.cpu().numpy())
    ev_b.close()
    # the final device latents through the device writer and a coded decode slot
    enc, dec = EncodeBatch(0), DecodeBatch(0)
    for p, d in zip(pics, devs):
        enc.add_device(p.geo.arch, p.geo.nn, p.ptrs(d), owner=d)
    enc.run(); enc.wait()
    for s, p in enumerate(pics):
        cc = enc.bytes(s)
        h2 = writer.parse_cc_header(cc)
        a, b = h2.n_bytes_header, h2.n_bytes_header + h2.nn_n_bytes
        dec.add(cc[:a], cc[a:b], cc[b:], p.geo.bd, p.geo.fdt)
    dec.run(); dec.wait()
    for s, (p, d) in enumerate(zip(pics, devs)):
        for got, want in zip(dec.planes(s), ev._dec.planes(s)):
            assert np.array_equal(got, want), p.geo.name
        for g, want in enumerate(p.grids(d)):
            assert np.array_equal(dec.latent(s, g), want), (p.geo.name, g)
        assert any(not np.array_equal(a_, b_) for a_, b_ in zip(p.grids(d), p.moved))  # the descent did move latents
    enc.close(); dec.close(); ev.close()


@pytest.mark.gpu
def test_host_candidates_are_refused(gpu, oracle):
    from cool_chic_amd import RdEvaluator

    pic = _picture(oracle, "odd18x65")
    dev = pic.device_latents()
    before = dev.cpu().numpy().copy()
    ev = RdEvaluator(0)
    ev.add(pic.geo.arch, pic.geo.nn, pic.ptrs(dev), pic.source, owner=dev)
    ev.add(pic.geo.arch, pic.geo.nn, pic.moved, pic.source)
    first = ev.evaluate(1e-3)
    with pytest.raises(ValueError):
        ev.descend(1e-3, max_steps=2)
    assert np.array_equal(dev.cpu().numpy(), before)
    again = ev.evaluate(1e-3)
    assert [(c.cost, c.bits, c.mse) for c in first] == [(c.cost, c.bits, c.mse) for c in again]
    ev.close()
