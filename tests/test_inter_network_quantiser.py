"""The q-step search for the two cool-chics of a P / B frame (cool_chic_amd/nnquant_inter.py).

CPU: the selection `search_steps_pair` equals an exhaustive reference descent over made-up costs.
GPU: frames of the video fixtures (a P frame of vid3_ldp, a B frame of vid5, a 4-tap P frame of vid5_w4, and a P frame of
vid3_hop, whose two cool-chics both have IFCE parameters) through
tests/inter_cases.py's parser.  The floats are the stream's own networks dequantised, the source is the frame's decoded planes
plus seeded +-3 LSB noise.  Yardsticks: InterRdEvaluator.evaluate of a pair of networks added ALONE for everything the search
prices, the CPU oracle for the stream written from the result.  Every comparison is of integers or of float64 bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_network_quantiser import TABLES, _rank, _u64

LMBDA = 1e-3
FRAMES = {"P": ("vid3_ldp", 1), "B": ("vid5", 2), "P4": ("vid5_w4", 1), "P_ifce": ("vid3_hop", 1)}   # (fixture, coding index)
SIZES = {"arm": 153, "ifce": 153, "upsampling": 13, "synthesis": 325}
GROUP = {"arm": 0, "ifce": 2, "upsampling": 4, "synthesis": 6}
FINEST = [f for _, f in TABLES]


# ---- CPU: the selection, on made-up costs ----------------------------------------------------------------------------------------
def _reference_descent(cost, feasible, n_bytes, has_ifce, sweeps):
    """Coordinate descent over both networks by exhaustive enumeration: per (role, module) the sorted list of every feasible pair
    under the stated order.  Returns (steps [2][8], the steps after every module, the cost after every module or None)."""
    steps = [list(FINEST), list(FINEST)]
    history, costs = [], []
    for _ in range(sweeps):
        before = [list(s) for s in steps]
        for role in range(2):
            for m in range(4):
                if m == 1 and not has_ifce[role]:
                    continue
                gw, gb = 2 * m, 2 * m + 1
                ranked = []
                for q_w in range(TABLES[gw][1], TABLES[gw][1] + TABLES[gw][0]):
                    for q_b in range(TABLES[gb][1], TABLES[gb][1] + TABLES[gb][0]):
                        s = [list(x) for x in steps]
                        s[role][gw], s[role][gb] = q_w, q_b
                        if feasible(s):
                            ranked.append((cost(s), n_bytes(s, role), -q_w, -q_b))
                if ranked:
                    _, _, w, b = sorted(ranked)[0]
                    steps[role][gw], steps[role][gb] = -w, -b
                history.append([list(s) for s in steps])
                costs.append(cost(steps) if feasible(steps) else None)
        if steps == before:
            break
    return steps, history, costs


def _pricer(cost, feasible, n_bytes):
    from cool_chic_amd.nnquant import Cell, module_cells

    def price(role, m, steps):
        cells = []
        for q_w, q_b in module_cells(m):
            s = [list(x) for x in steps]
            s[role][2 * m], s[role][2 * m + 1] = q_w, q_b
            ok = feasible(s)
            cells.append(Cell(q_w, q_b, ok, n_bytes(s, role), 0.0, 0.0, cost(s) if ok else float("nan")))
        return cells
    return price


def _check_against_reference(cost, feasible, n_bytes, has_ifce, sweeps):
    from cool_chic_amd.nnquant_inter import search_steps_pair

    told = []
    want, history, costs = _reference_descent(cost, feasible, n_bytes, has_ifce, sweeps)
    steps, tables = search_steps_pair(_pricer(cost, feasible, n_bytes), has_ifce, sweeps, lambda r, m, k: told.append((r, m, k)))
    assert steps == want and len(tables) == len(history)
    per_sweep = [(r, n) for r in range(2) for n in ("arm", "ifce", "upsampling", "synthesis") if n != "ifce" or has_ifce[r]]
    assert [(t.role, t.module) for t in tables] == per_sweep * (len(tables) // len(per_sweep))
    assert [t.sweep for t in tables] == [i // len(per_sweep) for i in range(len(tables))]
    assert told == [(t.role, "arm ifce upsampling synthesis".split().index(t.module), t.chosen) for t in tables if t.chosen is not None]
    # every table is the module's pairs, every choice its minimum under the tie-break, and the cost never rises
    last = None
    for t, after, c in zip(tables, history, costs):
        assert t.chosen == _rank(t.cells)
        if t.chosen is None:
            continue
        g = GROUP[t.module]
        assert (t.cells[t.chosen].q_w, t.cells[t.chosen].q_b) == (after[t.role][g], after[t.role][g + 1])
        assert t.cells[t.chosen].cost == c
        assert last is None or c <= last
        last = c
    return steps, tables


def test_pair_selection_equals_exhaustive_enumeration():
    from cool_chic_amd.nnquant import module_cells
    from cool_chic_amd.nnquant_inter import InterModuleTable, search_steps_pair

    assert InterModuleTable._fields == ("sweep", "role", "module", "cells", "chosen")
    rng = np.random.default_rng(19)
    at = lambda s, r, m: (s[r][2 * m] - TABLES[2 * m][1], s[r][2 * m + 1] - TABLES[2 * m + 1][1])  # noqa: E731
    # 1. a separable cost with many exact ties (few distinct values) and random byte counts: every tie-break is exercised, with
    #    feasibility masks that take most minima away; IFCE in both, in one only (either), in none; sweeps 1 and 3
    terms = [[rng.integers(0, 3, (TABLES[2 * m][0], TABLES[2 * m + 1][0])).astype(np.float64) for m in range(4)] for _ in range(2)]
    sizes = [[rng.integers(0, 2, (TABLES[2 * m][0], TABLES[2 * m + 1][0])) for m in range(4)] for _ in range(2)]
    blocked = [[rng.random(t.shape) < 0.4 for t in row] for row in terms]
    for brow, trow in zip(blocked, terms):
        for b, t in zip(brow, trow):
            b[t == t.min()] = rng.random(int((t == t.min()).sum())) < 0.7
            b[0, 0] = False  # (the start itself stays feasible)
    cost = lambda s: float(sum(terms[r][m][at(s, r, m)] for r in range(2) for m in range(4)))  # noqa: E731
    n_bytes = lambda s, role: int(sum(sizes[role][m][at(s, role, m)] for m in range(4)))         # noqa: E731
    for has_ifce in ((True, True), (True, False), (False, True), (False, False)):
        masked = lambda s: not any(blocked[r][m][at(s, r, m)] for r in range(2) for m in range(4) if m != 1 or has_ifce[r])  # noqa: E731
        for feasible in (lambda s: True, masked):
            for sweeps in (1, 3):
                steps, tables = _check_against_reference(cost, feasible, n_bytes, has_ifce, sweeps)
                assert all(t.chosen is not None and t.cells[t.chosen].feasible for t in tables)
                for r in range(2):
                    if not has_ifce[r]:
                        assert steps[r][2:4] == FINEST[2:4]
    # 2. a cost that couples the residue's ARM with the MOTION's synthesis: the second sweep changes the first module's choice
    coupled = lambda s: float(abs((s[0][0] + 8) - (s[1][6] + 12) // 2) + 0.25 * (s[1][6] + 12 - 9) ** 2 + abs(s[0][1] + 10)  # noqa: E731
                              + abs(s[1][7] + 20) + abs(s[0][6] + 5) + abs(s[1][0] + 3))
    free = lambda s: True          # noqa: E731
    nothing = lambda s, role: 0    # noqa: E731
    one, t1 = _check_against_reference(coupled, free, nothing, (True, False), 1)
    two, t2 = _check_against_reference(coupled, free, nothing, (True, False), 2)
    many, t9 = _check_against_reference(coupled, free, nothing, (True, False), 9)
    assert one[0][0] != two[0][0] and one[1][6] == two[1][6] and len(t1) == 7 and len(t2) == 14
    assert len(t9) == 21 and [t.sweep for t in t9] == [0] * 7 + [1] * 7 + [2] * 7  # stops after the sweep that changes nothing
    assert coupled(one) > coupled(two) >= coupled(many)
    # 3. a module without a feasible cell keeps its steps and chooses nothing: everything is infeasible while the motion cool-chic's
    #    synthesis weights are at their finest step - the whole residue cool-chic and three modules of the motion one wait
    held = lambda s: s[1][6] > -12  # noqa: E731
    steps, tables = _check_against_reference(coupled, held, nothing, (True, True), 2)
    assert [t.chosen is None for t in tables[:8]] == [True] * 7 + [False] and all(t.chosen is not None for t in tables[8:])
    assert all(not c.feasible and np.isnan(c.cost) for t in tables[:7] for c in t.cells)
    # a table that is not the module's pairs is refused; a pricing that fails ends the selection at once
    assert [len(module_cells(m)) for m in range(4)] == [153, 153, 13, 325]
    with pytest.raises(ValueError):
        search_steps_pair(lambda r, m, s: _pricer(coupled, free, nothing)(r, m, s)[:-1], (True, True), 1)
    with pytest.raises(ValueError):
        search_steps_pair(lambda r, m, s: _pricer(coupled, free, nothing)(r, m, s)[::-1], (True, True), 1)
    calls = []

    def failing(role, m, steps):
        calls.append((role, m))
        raise RuntimeError("stub")

    with pytest.raises(RuntimeError):
        search_steps_pair(failing, (True, True), 3)
    assert calls == [(0, 0)]


def test_the_search_is_exported():
    import cool_chic_amd
    from cool_chic_amd import nnquant_inter

    assert cool_chic_amd.InterNetworkQuantiser is nnquant_inter.InterNetworkQuantiser
    assert cool_chic_amd.QuantisedInterNetworks is nnquant_inter.QuantisedInterNetworks
    assert nnquant_inter.QuantisedInterNetworks._fields == ("residue", "motion", "candidate", "tables", "pricing")
    assert nnquant_inter.RoleNetwork._fields == ("header", "bytes_nn", "values")
    assert os.path.exists(os.path.join(ROOT, "tools", "quantise_video_networks.py"))


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cool_chic_amd import _lib

    _lib.lib()
    return torch


class _Case:
    """One inter frame of a video fixture: both cool-chics' latents on the device, the references as the library decodes them, a
    source (the frame's decoded planes plus seeded noise of a few LSB) and the floats the stream's own integers dequantise to."""

    def __init__(self, torch, key):
        import inter_cases as ic
        from cool_chic_amd import DecodeBatch, writer
        from cool_chic_amd.quality import _planes_to_frame_data

        self.name, self.k = FRAMES[key]
        self.parsed = ic.parse_video(self.name)
        fh, ccs, disp, ref_display = self.parsed[self.k]
        self.fh, self.display = fh, disp
        self.frame_type = int(fh.frame_type)
        assert self.frame_type == (2 if key == "B" else 1) and len(ccs) == 2
        self.bitdepth, self.fdt = int(fh.bitdepth), int(fh.frame_data_type)
        self.taps, self.gflow = int(fh.warp_filter_size), [int(v) for v in fh.global_flow][:4]
        planes = ic.decoded_planes(self.name)
        self.refs = [[p.clone() for p in planes[d]] for d in ref_display[:self.frame_type]]
        dec = DecodeBatch(0)
        for arch, hdr, nn, lat in ccs:
            dec.add(hdr, nn, lat, 0, 0)
        dec.run(); dec.wait()
        self.archs = [dec.header(i) for i in range(2)]
        self.nns = [ccs[i][2] for i in range(2)]
        self.host_latents = [[dec.latent(i, g) for g in range(int(self.archs[i].n_grids))] for i in range(2)]
        dec.close()
        self.latents = [[torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in row] for row in self.host_latents]
        self.ptrs = [[t.data_ptr() for t in row] for row in self.latents]
        rng = np.random.default_rng([len(self.name), self.k])
        own = [p.cpu().numpy() for p in planes[disp]]
        maxv = 2 ** self.bitdepth - 1
        self.source_planes = [np.clip(p.astype(np.int64) + rng.integers(-3, 4, p.shape), 0, maxv).astype(p.dtype) for p in own]
        self.source = _planes_to_frame_data(self.source_planes, self.bitdepth, ["rgb", "yuv420", "yuv444"][self.fdt])
        self.floats = [writer.dequantise_network(a, writer.network_values(a, nn)) for a, nn in zip(self.archs, self.nns)]
        self.has_ifce = [writer.network_layout(a)[2] > 0 for a in self.archs]
        self._searches = {}

    def search(self, archs=None, floats=None, key=None, **kw):
        from cool_chic_amd import InterNetworkQuantiser

        k = (key, tuple(sorted(kw.items())))
        if k not in self._searches:
            init = {a: kw.pop(a) for a in ("max_in_flight_bytes",) if a in kw}
            archs, floats = archs or self.archs, floats or self.floats
            self._searches[k] = InterNetworkQuantiser(0, **init).search(
                self.frame_type, (archs[0], floats[0], self.ptrs[0]), (archs[1], floats[1], self.ptrs[1]), self.refs, self.gflow, self.taps,
                self.source, LMBDA, owner=self.latents, **kw)
        return self._searches[k]

    def alone(self, nets):
        """InterRdEvaluator.evaluate of a pair of networks [(header, bytes_nn)] added alone."""
        from cool_chic_amd import InterRdEvaluator

        with InterRdEvaluator(0) as ev:
            ev.add(self.frame_type, (nets[0][0], nets[0][1], self.ptrs[0]), (nets[1][0], nets[1][1], self.ptrs[1]), self.refs, self.gflow,
                   self.taps, self.source, owner=self.latents)
            return ev.evaluate(LMBDA)[0]


_CASES = {}


@pytest.fixture
def case(gpu):
    def get(key):
        if key not in _CASES:
            _CASES[key] = _Case(gpu, key)
        return _CASES[key]
    return get


def _replay(tables):
    """[(table, steps [2][8] before the module was visited)], and the steps at the end."""
    steps = [list(FINEST), list(FINEST)]
    out = []
    for t in tables:
        out.append((t, [list(s) for s in steps]))
        if t.chosen is not None:
            g = GROUP[t.module]
            steps[t.role][g], steps[t.role][g + 1] = t.cells[t.chosen].q_w, t.cells[t.chosen].q_b
    return out, steps


def _expected_modules(c, sweeps=1):
    return [(r, n) for r in range(2) for n in ("arm", "ifce", "upsampling", "synthesis") if n != "ifce" or c.has_ifce[r]] * sweeps


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(FRAMES))
def test_meter_shortcuts_are_exact(case, key):
    """Every upsampling cell and at least 24 seeded cells of every other table of both roles, corners included, equal
    InterRdEvaluator.evaluate of that pair of networks added alone - mse, bits, cost as float64 bit for bit, and the payload size:
    running only the meter a module can change loses nothing, nor does scoring hundreds of candidates per launch."""
    from cool_chic_amd.nnquant import build_network

    c = case(key)
    res = c.search()
    assert [(t.role, t.module) for t in res.tables] == _expected_modules(c)
    rng = np.random.default_rng(23)
    for t, steps in _replay(res.tables)[0]:
        n, g = len(t.cells), GROUP[t.module]
        nb = TABLES[g + 1][0]
        feasible = [i for i, x in enumerate(t.cells) if x.feasible]
        if t.module == "upsampling":
            which = list(range(n))
        else:
            pool = [i for i in feasible if i not in (0, nb - 1, n - nb, n - 1)]
            which = sorted({0, nb - 1, n - nb, n - 1} | set(rng.choice(pool, 24, replace=False).tolist()))
        checked = 0
        for i in which:
            cell = t.cells[i]
            s = [list(x) for x in steps]
            s[t.role][g], s[t.role][g + 1] = cell.q_w, cell.q_b
            nets = [build_network(c.archs[r], c.floats[r], s[r]) for r in range(2)]
            assert all(x is not None and x.feasible for x in nets) and cell.feasible, (t.role, t.module, i)
            want = c.alone([(x.header, x.bytes_nn) for x in nets])
            assert cell.n_bytes_nn == len(nets[t.role].bytes_nn) == want.rates[t.role].n_bytes_nn
            assert _u64([cell.mse, cell.bits, cell.cost]) == _u64([want.mse, want.bits, want.cost]), (t.role, t.module, cell.q_w, cell.q_b)
            checked += 1
        assert checked >= (13 if t.module == "upsampling" else 24)
    last = res.tables[-1]
    assert _u64([res.candidate.mse, res.candidate.bits, res.candidate.cost]) == _u64(list(last.cells[last.chosen][4:7]))


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(FRAMES))
def test_tables_are_complete_and_the_choice_is_their_minimum(case, key):
    from cool_chic_amd.nnquant import module_cells

    c = case(key)
    res = c.search()
    replayed, steps = _replay(res.tables)
    costs = []
    for t, _ in replayed:
        m = "arm ifce upsampling synthesis".split().index(t.module)
        assert len(t.cells) == SIZES[t.module] and [(x.q_w, x.q_b) for x in t.cells] == module_cells(m)
        assert t.chosen == _rank(t.cells) and t.cells[t.chosen].feasible
        assert all(np.isfinite([x.mse, x.bits, x.cost]).all() for x in t.cells if x.feasible)
        costs.append(t.cells[t.chosen].cost)
    assert all(b <= a for a, b in zip(costs, costs[1:])), costs  # the cost after every module is <= the cost before it
    for r, net in enumerate(res.roles):
        assert list(net.header.nn_q_step_log2) == steps[r]
        assert net.header.nn_n_bytes == len(net.bytes_nn) <= 16383
    assert len(res.pricing) == len(res.tables) and all(0.0 <= h.build_seconds <= h.seconds for h in res.pricing)
    # the result is no worse than the pair at the finest steps, which is every table's first cell while nothing has moved
    assert costs[-1] <= res.tables[0].cells[0].cost


@pytest.mark.gpu
def test_sweeps_and_chunking(case):
    from cool_chic_amd.nnquant import NetworkQuantiser

    c = case("P")
    one = c.search()
    two = c.search(sweeps=2)
    n_mod = len(_expected_modules(c))
    assert n_mod < len(two.tables) <= 2 * n_mod and [(t.role, t.module) for t in two.tables] == _expected_modules(c, 2)[:len(two.tables)]
    within = [t.cells[t.chosen].cost for t in two.tables]
    assert all(b <= a for a, b in zip(within, within[1:])) and within[-1] <= one.candidate.cost  # sweeps = 2 never raises the cost
    for a, b in zip(two.tables, one.tables):  # the first sweep is the search with one sweep
        assert a.chosen == b.chosen and all(x[:4] == y[:4] and _u64(list(x[4:])) == _u64(list(y[4:])) for x, y in zip(a.cells, b.cells))
    # chunks of 1, of 7 and of everything: the same tables, bit for bit
    sb = max(NetworkQuantiser.slot_bytes(a, m) for a in c.archs for m in range(4))
    for budget, want_chunk in ((1, 1), (7 * sb + sb // 2, 7)):
        other = c.search(max_in_flight_bytes=budget)
        assert min(h.chunk for h in other.pricing) == want_chunk and min(h.chunk for h in one.pricing) >= 325
        for r in range(2):
            assert other.roles[r].bytes_nn == one.roles[r].bytes_nn and bytes(other.roles[r].header) == bytes(one.roles[r].header)
        assert len(other.tables) == len(one.tables)
        for a, b in zip(other.tables, one.tables):
            assert (a.role, a.module, a.chosen, len(a.cells)) == (b.role, b.module, b.chosen, len(b.cells))
            for x, y in zip(a.cells, b.cells):
                assert x[:4] == y[:4] and _u64(list(x[4:])) == _u64(list(y[4:]))


@pytest.mark.gpu
def test_an_infeasible_cell_is_recorded_and_never_chosen(case):
    """The residue cool-chic with a wide synthesis (two hidden layers of 64) and seeded normal synthesis weights scaled until the
    network at the finest steps no longer fits the header's 14-bit nn_n_bytes: the start is infeasible, so nothing of the
    residue's ARM (and IFCE, upsampling) can be priced while the synthesis holds it back - those tables are all NaN and choose
    nothing; the synthesis table records the oversized cells with their size and NaN prices and chooses a feasible one; the motion
    cool-chic is then searched against it; the second sweep prices the residue's other modules."""
    from cool_chic_amd import writer
    from cool_chic_amd.nnquant import build_network

    c = case("P")
    donor = c.archs[0]
    out_c = int(donor.out_channels)
    arch = writer.derive_arch(donor, syn_layers=[(64, 1, 0, 1), (64, 1, 0, 1), (out_c, 1, 0, 0)])
    layout, own = writer.network_layout(arch), writer.network_layout(donor)
    assert layout[:6] == own[:6] and layout[6] >= 4800 and int(arch.out_channels) == out_c
    at = np.cumsum([0] + layout)
    x = np.zeros(sum(layout), np.float32)
    x[:at[6]] = c.floats[0][:at[6]]
    x[at[6]:at[7]] = (np.random.default_rng(7).standard_normal(layout[6]) / 64.0).astype(np.float32)
    for _ in range(40):
        net = build_network(arch, x, FINEST)
        if net is not None and len(net.bytes_nn) > 16383:
            break
        x[at[6]:at[7]] *= 2.0
    assert net is not None and not net.feasible and len(net.bytes_nn) > 16383
    res = c.search(archs=[arch, c.archs[1]], floats=[x, c.floats[1]], key="wide", sweeps=2)
    first = [t for t in res.tables if t.sweep == 0 and t.role == 0]
    assert [t.module for t in first][-1] == "synthesis"
    for t in first[:-1]:
        assert t.chosen is None and all(not cell.feasible and np.isnan([cell.mse, cell.bits, cell.cost]).all() for cell in t.cells)
    syn = first[-1]
    bad = [i for i, cell in enumerate(syn.cells) if not cell.feasible]
    assert 0 in bad and 1 <= len(bad) < 325
    assert all(syn.cells[i].n_bytes_nn > 16383 and np.isnan([syn.cells[i].mse, syn.cells[i].bits, syn.cells[i].cost]).all() for i in bad)
    assert all(cell.n_bytes_nn <= 16383 for cell in syn.cells if cell.feasible)
    assert syn.chosen == _rank(syn.cells) and syn.chosen not in bad
    for t in res.tables[len(first):]:
        assert t.chosen is not None and t.cells[t.chosen].feasible and t.cells[t.chosen].n_bytes_nn <= 16383
    assert any(t.sweep == 1 and t.role == 0 and t.module == "arm" for t in res.tables)
    # a checked cell of the synthesis table, priced while the start was infeasible (both meters ran), and the result
    _, steps = _replay(res.tables)
    for t, before in _replay(res.tables)[0]:
        if t is syn:
            cell = syn.cells[syn.chosen]
            s = list(before[0])
            s[6], s[7] = cell.q_w, cell.q_b
            nets = [build_network(arch, x, s), build_network(c.archs[1], c.floats[1], before[1])]
            want = c.alone([(n.header, n.bytes_nn) for n in nets])
            assert _u64([cell.mse, cell.bits, cell.cost]) == _u64([want.mse, want.bits, want.cost])
    assert list(res.residue.header.nn_q_step_log2) == steps[0] and len(res.residue.bytes_nn) <= 16383
    want = c.alone([(n.header, n.bytes_nn) for n in res.roles])
    last = res.tables[-1]
    assert _u64([res.candidate.cost]) == _u64([want.cost]) == _u64([last.cells[last.chosen].cost])


def _write_stream(c, nets):
    """The fixture's stream with the case's frame written from `nets` [(header, bytes_nn)] and its unchanged latents."""
    from cool_chic_amd import writer
    from oracle import oracle_py as oracle

    with open(os.path.join(GOLDEN, c.name + ".cool"), "rb") as f:
        bs = f.read()
    vh, frames = oracle.split_stream(bs)
    out = [writer.video_header_bytes(vh.n_frames, list(vh.intra_pos[:vh.n_intras]), list(vh.p_pos[:vh.n_p_frames]))]
    for k, (fh, ccs) in enumerate(frames):
        out.append(writer.frame_header_bytes(fh.display_index, "IPB"[fh.frame_type], fh.frame_data_type, fh.bitdepth, list(fh.index_references[:fh.n_refs]),
                                             list(fh.global_flow[:2 * fh.n_refs]), fh.warp_filter_size if fh.frame_type else 0))
        for i, triple in enumerate(ccs):
            out.append(writer.encode_coolchic(nets[i][0], nets[i][1], c.host_latents[i]) if k == c.k else b"".join(triple))
    return b"".join(out)


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(FRAMES))
def test_end_to_end_through_the_oracle(case, oracle, key):
    """The frame written with the chosen networks and the unchanged latents: the CPU oracle decodes the stream, the planes' squared
    error against the source and the stream's byte counts reproduce the result's candidate."""
    from cool_chic_amd import writer

    c = case(key)
    res = c.search()
    same = _write_stream(c, [(a, nn) for a, nn in zip(c.archs, c.nns)])
    with open(os.path.join(GOLDEN, c.name + ".cool"), "rb") as f:
        assert same == f.read()  # (the rewriting itself changes nothing)
    stream = _write_stream(c, [(n.header, n.bytes_nn) for n in res.roles])
    frames = oracle.decode_video(stream)
    frame = frames[c.display]
    sse = [int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum()) for a, b in zip(frame["planes"], c.source_planes)]
    assert sse == list(res.candidate.quality.sse) and [p.size for p in frame["planes"]] == list(res.candidate.quality.n)
    _, ccs = oracle.split_stream(stream)[1][c.k]
    for r, (hdr, nn, payload) in enumerate(ccs):
        net = res.roles[r]
        assert nn == net.bytes_nn and len(nn) == net.header.nn_n_bytes == res.candidate.rates[r].n_bytes_nn
        assert len(hdr) == res.candidate.rates[r].n_bytes_header
        h2 = writer.parse_cc_header(hdr)
        assert list(h2.nn_q_step_log2) == list(net.header.nn_q_step_log2) and list(h2.nn_expgol_cnt) == list(net.header.nn_expgol_cnt)
        assert np.array_equal(oracle.decode_coolchic(hdr, nn, payload, stop_after_entropy=True)["nn_ints"], net.values)
    assert res.candidate.bits == sum(x.total_bits for x in res.candidate.rates) + 8.0 * sum(len(h) + len(n) for h, n, _ in ccs)


@pytest.mark.gpu
def test_the_tool(gpu, oracle, tmp_path):
    """tools/quantise_video_networks.py on vid3_ldp (I P P) in a child process: exit 0 (its decode-back assertion inside), every
    frame is reported before and after, and the stream it wrote decodes (the oracle) with networks that fit their headers."""
    name = "vid3_ldp"
    with open(os.path.join(GOLDEN, name + ".cool"), "rb") as f:
        bs = f.read()
    rng = np.random.default_rng(12)
    decoded = oracle.decode_video(bs)
    yuv, out = tmp_path / "source.yuv", tmp_path / "out.cool"
    with open(yuv, "wb") as f:
        for frame in decoded:  # display order
            for p in frame["planes"]:
                f.write(np.clip(p.astype(np.int64) + rng.integers(-3, 4, p.shape), 0, 255).astype(np.uint8).tobytes())
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "quantise_video_networks.py"), os.path.join(GOLDEN, name + ".cool"), str(yuv),
                        str(out), "--lmbda", "1e-3"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0
    assert r.stdout.count("before:") == 3 and r.stdout.count("after:") == 3 and "frame 0 (I)" in r.stdout and "frame 2 (P)" in r.stdout
    back = oracle.decode_video(out.read_bytes())
    assert len(back) == 3 and [[p.shape for p in f["planes"]] for f in back] == [[p.shape for p in f["planes"]] for f in decoded]
    for _, ccs in oracle.split_stream(out.read_bytes())[1]:
        assert all(0 < len(nn) <= 16383 for _, nn, _ in ccs)
