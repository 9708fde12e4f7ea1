"""The search over the networks' quantisation steps (cool_chic_amd/nnquant.py) and its host primitives
(ccd_network_values, ccd_quantise_network, ccd_network_best_expgol).

Yardsticks: the oracle's integers and planes, numpy's rint, a Python count of Exp-Golomb lengths, exhaustive enumeration for
the selection, and RdEvaluator.evaluate of a candidate added ALONE for everything the search prices.  Every comparison is of
integers or of float64 bit for bit."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import IMAGE_STREAMS, ROOT, VIDEO_STREAMS, load_golden

ERR_VALUE, ERR_ARG = -2, -7
TABLES = [(9, -8), (17, -16), (9, -8), (17, -16), (13, -12), (1, 0), (13, -12), (25, -24)]  # the issue's: (count, first log2) per group
GPU_IMAGES = ["odd18x65", "odd100x37", "rgb192", "cr192", "yuv420_8b", "yuv444_10b"]
IFCE_CASE = "ifce3_15_18x65_s6_i3_h3"    # tests/arm_layouts.py: three IFCE features, on the coarse grids only (the fixtures: on every grid)
NO_IFCE_CASE = "arm_s1_i0_h0"            # no IFCE at all, and the smallest ARM: the search skips the module
GPU_CASES = GPU_IMAGES + [IFCE_CASE, NO_IFCE_CASE]
FAT_ARM_CASE = "arm_s40_i24_h2"          # 64 ARM inputs, two hidden layers: 8 448 ARM weights, enough for a payload over 16 383 bytes


def _cool_chics(oracle, name):
    """[(header bytes, nn bytes, latent bytes)] of every cool-chic of a fixture."""
    _, frames = oracle.split_stream(load_golden(name)[0])
    return [cc for _, ccs in frames for cc in ccs]


_ORACLE_INTS = {}


def _all_cool_chics(oracle):
    """(label, parsed header, nn bytes, the ORACLE's integers) of every cool-chic of every golden fixture; decoded once."""
    from cool_chic_amd import writer

    for name in IMAGE_STREAMS + VIDEO_STREAMS:
        for k, (hdr, nn, lat) in enumerate(_cool_chics(oracle, name)):
            if (name, k) not in _ORACLE_INTS:
                _ORACLE_INTS[(name, k)] = oracle.decode_coolchic(hdr, nn, lat, stop_after_entropy=True)["nn_ints"]
            yield f"{name}.cc{k}", writer.parse_cc_header(hdr), nn, _ORACLE_INTS[(name, k)]


def _u64(x):
    return np.asarray(x, np.float64).view(np.uint64).tolist()


# ---- CPU -------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    from cool_chic_amd import _lib, writer
    from cool_chic_amd._lib import CCHeader, lib

    with open(os.path.join(ROOT, "include", "ccd.h")) as f:
        header = f.read()
    for decl in ("int64_t ccd_network_values(const ccd_cc_header* arch, const uint8_t* bytes_nn, size_t n_nn, int32_t* values, int64_t cap);",
                 "int ccd_quantise_network(const ccd_cc_header* arch, const float* x, int64_t n_values, const int32_t q_step_log2[8],",
                 "int ccd_network_best_expgol(const ccd_cc_header* arch, const int32_t* values, int64_t n_values, int32_t order[8],"):
        assert decl in header
    assert "int ccd_q_step_table(int group, int32_t* log2_first);" in header
    for name in ("ccd_network_values", "ccd_quantise_network", "ccd_network_best_expgol", "ccd_q_step_table"):
        assert name in _lib.SIGNATURES and getattr(lib(), name) is not None
    assert all(hasattr(writer, f) for f in ("network_values", "quantise_network", "dequantise_network", "best_expgol"))
    import cool_chic_amd

    assert cool_chic_amd.NetworkQuantiser.__name__ == "NetworkQuantiser" and cool_chic_amd.QuantisedNetwork.__name__ == "QuantisedNetwork"
    assert hasattr(cool_chic_amd.NetworkQuantiser, "search")
    # null arguments: CCD_ERR_ARG before anything is read (the buffers that stand for the others are never looked at)
    L = lib()
    arch = CCHeader()   # all zero: anything that read it would answer CCD_ERR_VALUE
    buf = np.zeros(16, np.int32)
    p = buf.ctypes.data
    assert L.ccd_network_values(None, b"\x00", 1, p, 16) == ERR_ARG
    assert L.ccd_network_values(C.byref(arch), None, 0, p, 16) == ERR_ARG
    assert L.ccd_network_values(C.byref(arch), b"\x00", 1, None, 16) == ERR_ARG
    assert L.ccd_quantise_network(None, p, 16, p, p) == ERR_ARG
    assert L.ccd_quantise_network(C.byref(arch), None, 16, p, p) == ERR_ARG
    assert L.ccd_quantise_network(C.byref(arch), p, 16, None, p) == ERR_ARG
    assert L.ccd_quantise_network(C.byref(arch), p, 16, p, None) == ERR_ARG
    assert L.ccd_network_best_expgol(None, p, 16, p, p) == ERR_ARG
    assert L.ccd_network_best_expgol(C.byref(arch), None, 16, p, p) == ERR_ARG
    assert L.ccd_network_best_expgol(C.byref(arch), p, 16, None, p) == ERR_ARG
    assert L.ccd_network_best_expgol(C.byref(arch), p, 16, p, None) == ERR_ARG
    assert not buf.any()
    # the header's step tables, from the library
    first = C.c_int32(99)
    assert [(L.ccd_q_step_table(g, C.byref(first)), first.value) for g in range(8)] == TABLES
    assert L.ccd_q_step_table(-1, C.byref(first)) == L.ccd_q_step_table(8, C.byref(first)) == L.ccd_q_step_table(0, None) == ERR_ARG


def test_network_values_are_the_oracles(oracle):
    from cool_chic_amd import writer
    from cool_chic_amd._lib import CCHeader

    n = 0
    for what, arch, nn, stored in _all_cool_chics(oracle):
        got = writer.network_values(arch, nn)
        assert got.dtype == np.int32 and np.array_equal(got, stored), what
        a = CCHeader.from_buffer_copy(bytes(arch))
        assert writer.encode_network(a, got) == nn and (a.nn_n_bytes, a.nn_n_bit_pad) == (arch.nn_n_bytes, arch.nn_n_bit_pad), what
        n += 1
    assert n >= len(IMAGE_STREAMS) + 2 * len(VIDEO_STREAMS)
    # a buffer that is too small is an argument error and is not written to
    from cool_chic_amd._lib import lib

    small = np.full(4, 77, np.int32)
    assert lib().ccd_network_values(C.byref(arch), nn, len(nn), small.ctypes.data, 4) == ERR_ARG and (small == 77).all()


def _arch(oracle, name="rgb192"):
    from cool_chic_amd import writer

    hdr, nn, _ = _cool_chics(oracle, name)[0]
    arch = writer.parse_cc_header(hdr)
    return arch, nn, writer.network_layout(arch)


def _rint_reference(x, layout, steps):
    q = np.repeat(np.ldexp(np.float32(1), np.asarray(steps, np.int32)).astype(np.float32), layout)
    return np.rint((x / q).astype(np.float32))


def test_quantise_network_is_rint(oracle):
    from cool_chic_amd import writer
    from cool_chic_amd._lib import CcdError

    arch, _, layout = _arch(oracle)
    total = sum(layout)
    rng = np.random.default_rng(418)
    first = [t[1] for t in TABLES]
    last = [t[1] + t[0] - 1 for t in TABLES]
    assert [list(writer.q_step_range(g)) for g in range(8)] == [list(range(f, f + n)) for n, f in TABLES]
    for steps in (first, last, [int(rng.integers(f, l + 1)) for f, l in zip(first, last)]):
        q = np.repeat(np.ldexp(np.float32(1), np.asarray(steps, np.int32)).astype(np.float32), layout)
        x = (rng.standard_normal(total) * rng.choice([1e-3, 1.0, 50.0], total)).astype(np.float32)
        k = rng.integers(-40, 41, total)
        ties = rng.random(total) < 0.3               # exact ties of both signs: (k + 0.5) q
        x[ties] = ((k[ties] + 0.5) * q[ties].astype(np.float64)).astype(np.float32)
        x[rng.random(total) < 0.05] = 0.0
        x[rng.random(total) < 0.02] = -0.0
        edge = rng.random(total) < 0.05              # near int32's edge: the largest floats below 2^31, and -2^31 itself
        x[edge] = (rng.choice([2147483520.0, -2147483648.0, 2147483392.0, -2147483520.0], int(edge.sum())) * q[edge].astype(np.float64)).astype(np.float32)
        want = _rint_reference(x, layout, steps)
        assert (np.abs(want[ties]) % 2 == 0).any() and (want[ties] > 0).any() and (want[ties] < 0).any()
        assert want.min() == -2147483648.0 and want.max() == 2147483520.0
        got = writer.quantise_network(arch, x, steps)
        assert got.dtype == np.int32 and np.array_equal(got.astype(np.int64), want.astype(np.int64)), steps
    # refusals: a step outside its group's table, a non-finite value, a result outside int32, a wrong count
    ok = np.zeros(total, np.float32)
    for g in range(8):
        for bad in (first[g] - 1, last[g] + 1):
            steps = list(first)
            steps[g] = bad
            with pytest.raises(CcdError) as e:
                writer.quantise_network(arch, ok, steps)
            assert e.value.code == ERR_VALUE, (g, bad)
    for bad in (np.inf, -np.inf, np.nan):
        for at in (0, total - 1):
            x = ok.copy()
            x[at] = bad
            with pytest.raises(CcdError) as e:
                writer.quantise_network(arch, x, first)
            assert e.value.code == ERR_VALUE
    starts = np.cumsum([0] + layout[:-1])
    for g in (0, 7):
        for v in (2147483648.0, -2147483904.0, 3.0e38):
            x = ok.copy()
            x[starts[g]] = np.float32(v * 2.0 ** first[g]) if v < 1e38 else np.float32(v)
            with pytest.raises(CcdError) as e:
                writer.quantise_network(arch, x, first)
            assert e.value.code == ERR_VALUE, (g, v)
    with pytest.raises(CcdError) as e:
        writer.quantise_network(arch, ok[:-1], first)
    assert e.value.code == ERR_ARG


def test_quantise_inverts_dequantise_at_every_step(oracle):
    from cool_chic_amd import writer

    for what, arch, nn, ints in _all_cool_chics(oracle):
        own = list(arch.nn_q_step_log2)
        assert np.array_equal(writer.quantise_network(arch, writer.dequantise_network(arch, ints), own), ints), what
        for g in range(8):
            for q in writer.q_step_range(g):
                steps = list(own)
                steps[g] = q
                x = writer.dequantise_network(arch, ints, steps)
                assert x.dtype == np.float32 and np.array_equal(writer.quantise_network(arch, x, steps), ints), (what, g, q)


def _expgol_bits(v, k):
    """Length of the order-k Exp-Golomb code of the signed value v (expgolomb.py:45-62), counted in Python integers."""
    u = -2 * v if v <= 0 else 2 * v - 1
    return 2 * ((u + (1 << k)).bit_length() - 1) - k + 1


def _best_orders(values, layout):
    out, at = [], 0
    for n in layout:
        group = [int(v) for v in values[at:at + n]]
        at += n
        bits = [sum(_expgol_bits(v, k) for v in group) for k in range(13)]
        k = min(range(13), key=lambda k: (bits[k], k))
        out.append((k, bits[k]))
    return [o for o, _ in out], [b for _, b in out]


def test_best_expgol_is_the_count(oracle):
    from cool_chic_amd import writer
    from cool_chic_amd._lib import CCHeader

    cases = [(w, a, ints) for w, a, _, ints in _all_cool_chics(oracle)]
    arch, _, layout = _arch(oracle)
    rng = np.random.default_rng(419)
    total = sum(layout)
    for scale in (0.3, 3.0, 40.0, 3000.0, 2.0e8):
        cases.append((f"seeded {scale}", arch, np.clip(np.rint(rng.laplace(size=total) * scale), -2 ** 31, 2 ** 31 - 1).astype(np.int32)))
    edge = np.zeros(total, np.int32)
    edge[:4] = [2 ** 31 - 1, -2 ** 31, 1, -1]
    cases.append(("int32 edge", arch, edge))
    seen = set()
    for what, a, ints in cases:
        lay = writer.network_layout(a)
        want = _best_orders(ints, lay)
        got = writer.best_expgol(a, ints)
        assert got == want, what
        assert all(o == 0 and b == 0 for o, b, n in zip(got[0], got[1], lay) if n == 0), what
        seen.update(got[0])
        h = CCHeader.from_buffer_copy(bytes(a))
        for g in range(8):
            h.nn_expgol_cnt[g] = got[0][g]
        nn = writer.encode_network(h, ints)
        n_bits = sum(got[1])
        assert len(nn) == -(-n_bits // 8) and h.nn_n_bit_pad == 8 * len(nn) - n_bits and h.nn_n_bytes == len(nn), what
        assert np.array_equal(writer.network_values(h, nn), ints), what
    assert len(seen) >= 5 and 12 in seen


def test_the_header_writer_truncates_an_overlong_payload(oracle):
    """Why the search itself must refuse a payload beyond 16 383 bytes: the header writer stores the low 14 bits."""
    from cool_chic_amd import writer
    from cool_chic_amd._lib import CCHeader

    arch, _, _ = _arch(oracle)
    h = CCHeader.from_buffer_copy(bytes(arch))
    h.nn_n_bytes = writer.MAX_NN_BYTES + 1
    assert writer.MAX_NN_BYTES == 16383 and writer.parse_cc_header(writer.cc_header_bytes(h)).nn_n_bytes == 0


# ---- the selection, on made-up costs -------------------------------------------------------------------------------------
def _reference_descent(cost, feasible, n_bytes, has_ifce, sweeps):
    """Coordinate descent by exhaustive enumeration: per module the sorted list of every feasible pair under the stated order."""
    steps = [f for _, f in TABLES]
    history = []
    for _ in range(sweeps):
        before = list(steps)
        for m in range(4):
            if m == 1 and not has_ifce:
                continue
            gw, gb = 2 * m, 2 * m + 1
            ranked = []
            for q_w in range(TABLES[gw][1], TABLES[gw][1] + TABLES[gw][0]):
                for q_b in range(TABLES[gb][1], TABLES[gb][1] + TABLES[gb][0]):
                    s = list(steps)
                    s[gw], s[gb] = q_w, q_b
                    if feasible(s):
                        ranked.append((cost(s), n_bytes(s), -q_w, -q_b))
            if ranked:
                _, _, w, b = sorted(ranked)[0]
                steps[gw], steps[gb] = -w, -b
            history.append(list(steps))
        if steps == before:
            break
    return steps, history


def _pricer(cost, feasible, n_bytes):
    from cool_chic_amd.nnquant import Cell, module_cells

    def price(m, steps):
        cells = []
        for q_w, q_b in module_cells(m):
            s = list(steps)
            s[2 * m], s[2 * m + 1] = q_w, q_b
            ok = feasible(s)
            cells.append(Cell(q_w, q_b, ok, n_bytes(s), 0.0, 0.0, cost(s) if ok else float("nan")))
        return cells
    return price


def test_selection_equals_exhaustive_enumeration():
    from cool_chic_amd.nnquant import module_cells, search_steps

    assert [len(module_cells(m)) for m in range(4)] == [153, 153, 13, 325]
    finest = [f for _, f in TABLES]
    rng = np.random.default_rng(5)
    # 1. a separable cost with many exact ties (few distinct values): per module the global optimum, every tie-break exercised
    terms = [rng.integers(0, 3, (TABLES[2 * m][0], TABLES[2 * m + 1][0])).astype(np.float64) for m in range(4)]
    sizes = [rng.integers(0, 2, (TABLES[2 * m][0], TABLES[2 * m + 1][0])) for m in range(4)]
    at = lambda s, m: (s[2 * m] - TABLES[2 * m][1], s[2 * m + 1] - TABLES[2 * m + 1][1])  # noqa: E731
    cost = lambda s: float(sum(terms[m][at(s, m)] for m in range(4)))                      # noqa: E731
    n_bytes = lambda s: int(sum(sizes[m][at(s, m)] for m in range(4)))                     # noqa: E731
    blocked = [rng.random(t.shape) < 0.4 for t in terms]
    for b, t in zip(blocked, terms):  # every minimum of the cost is infeasible in one module: the choice must step around them
        b[t == t.min()] = rng.random(int((t == t.min()).sum())) < 0.7
    blocked[0][0, 0] = blocked[1][0, 0] = blocked[2][0, 0] = blocked[3][0, 0] = False  # (the start itself stays feasible)
    for has_ifce in (True, False):
        for feasible in (lambda s: True, lambda s: not any(blocked[m][at(s, m)] for m in range(4) if m != 1 or has_ifce)):
            want, history = _reference_descent(cost, feasible, n_bytes, has_ifce, 3)
            steps, tables = search_steps(_pricer(cost, feasible, n_bytes), has_ifce, 3)
            assert steps == want and len(tables) == len(history) == 2 * (4 if has_ifce else 3)
            assert [t.module for t in tables[:4 if has_ifce else 3]] == [n for n in ("arm", "ifce", "upsampling", "synthesis") if has_ifce or n != "ifce"]
            assert all(t.chosen is not None and t.cells[t.chosen].feasible for t in tables)
            if not has_ifce:
                assert steps[2:4] == finest[2:4]
            # separable: the descent's end is the global optimum, module by module
            for m in range(4):
                if m == 1 and not has_ifce:
                    continue
                best = min((terms[m][i, j], sizes[m][i, j], -i, -j) for i in range(terms[m].shape[0]) for j in range(terms[m].shape[1])
                           if feasible([TABLES[g][1] + (i if g == 2 * m else j if g == 2 * m + 1 else 0) for g in range(8)]))
                assert at(steps, m) == (-best[2], -best[3]), (m, has_ifce)
    # 2. a cost that couples the ARM's weight step with the synthesis': the second sweep changes the FIRST module's choice
    coupled = lambda s: float(abs((s[0] + 8) - (s[6] + 12) // 2) + 0.25 * (s[6] + 12 - 9) ** 2 + abs(s[1] + 10) + abs(s[7] + 20))  # noqa: E731
    one, t1 = search_steps(_pricer(coupled, lambda s: True, lambda s: 0), True, 1)
    two, t2 = search_steps(_pricer(coupled, lambda s: True, lambda s: 0), True, 2)
    many, t9 = search_steps(_pricer(coupled, lambda s: True, lambda s: 0), True, 9)
    assert one[0] != two[0] and one[6] == two[6] and len(t1) == 4 and len(t2) == 8
    assert two == _reference_descent(coupled, lambda s: True, lambda s: 0, True, 2)[0]
    assert many == _reference_descent(coupled, lambda s: True, lambda s: 0, True, 9)[0] and len(t9) == 12  # stops after the sweep that changes nothing
    assert [t.sweep for t in t9] == [0] * 4 + [1] * 4 + [2] * 4
    per_sweep = [coupled([c for c in _reference_descent(coupled, lambda s: True, lambda s: 0, True, k)[0]]) for k in (1, 2, 3)]
    assert per_sweep[0] > per_sweep[1] >= per_sweep[2]
    # 3. a module without a feasible cell keeps its steps and chooses nothing
    no_arm = lambda s: s[6] > -12  # noqa: E731  (everything is infeasible while the synthesis weights are at their finest step)
    steps, tables = search_steps(_pricer(coupled, no_arm, lambda s: 0), True, 2)
    assert [t.chosen is None for t in tables[:4]] == [True, True, True, False] and all(t.chosen is not None for t in tables[4:])
    assert steps == _reference_descent(coupled, no_arm, lambda s: 0, True, 2)[0]
    # a table that is not the module's pairs is refused
    with pytest.raises(ValueError):
        search_steps(lambda m, s: _pricer(coupled, no_arm, lambda s: 0)(m, s)[:-1], True, 1)


def test_only_refusals_of_a_network_make_a_candidate_infeasible(oracle, monkeypatch):
    """CCD_ERR_VALUE / INVALID_DATA / UNSUPPORTED refuse the network: infeasible.  Out of memory, a HIP error, a wrong argument say
    nothing about the candidate: they are raised, from an add (refused()), from building a candidate, and through the selection."""
    from cool_chic_amd import nnquant, writer
    from cool_chic_amd._lib import CcdError

    def raising(code):
        def call(*args, **kwargs):
            raise CcdError(code, "stub")
        return call

    assert nnquant.refused(lambda a, b=0: a + b, 2, b=3) == (5, False)
    for code in (-2, -3, -4):
        assert nnquant.refused(raising(code), 1) == (None, True)
    for code in (-1, -5, -6, -7):
        with pytest.raises(CcdError) as e:
            nnquant.refused(raising(code), 1)
        assert e.value.code == code
    arch, nn, _ = _arch(oracle)
    floats = writer.dequantise_network(arch, writer.network_values(arch, nn))
    own = list(arch.nn_q_step_log2)
    assert nnquant.build_network(arch, floats, own).feasible
    assert nnquant.build_network(arch, floats * np.float32(3e38), own) is None            # a value outside int32: refused, infeasible
    for name in ("quantise_network", "best_expgol", "encode_network"):
        for code in (-5, -6, -7):
            with monkeypatch.context() as mp:
                mp.setattr(writer, name, raising(code))
                with pytest.raises(CcdError) as e:
                    nnquant.build_network(arch, floats, own)
                assert e.value.code == code, (name, code)
    with monkeypatch.context() as mp:
        mp.setattr(writer, "fits_fast_path", raising(-5))
        assert nnquant.build_network(arch, floats, own).feasible                          # not asked for: not called
        with pytest.raises(CcdError):
            nnquant.build_network(arch, floats, own, fast_path_only=True)
        mp.setattr(writer, "fits_fast_path", raising(-3))
        assert not nnquant.build_network(arch, floats, own, fast_path_only=True).feasible
        mp.setattr(writer, "fits_fast_path", lambda *a: False)
        assert not nnquant.build_network(arch, floats, own, fast_path_only=True).feasible
    # a pricing that fails ends the selection at once, with that error
    calls = []

    def price(m, steps):
        calls.append(m)
        raise CcdError(-5, "stub")

    with pytest.raises(CcdError) as e:
        nnquant.search_steps(price, True, 3)
    assert e.value.code == -5 and calls == [0]


# ---- GPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cool_chic_amd import _lib

    _lib.lib()
    return torch


class _Case:
    """A cool-chic with its latents on the device, a source (the decoded planes plus seeded noise of a few LSB) and the float
    parameters its own integers dequantise to."""

    def __init__(self, torch, oracle, name):
        from cool_chic_amd import DecodeBatch, writer
        from cool_chic_amd.quality import _planes_to_frame_data

        if name in GPU_IMAGES:
            _, frames = oracle.split_stream(load_golden(name)[0])
            (fh, ccs), = frames
            self.hdr, self.nn, payload = ccs[0]
            self.bitdepth, self.fdt = int(fh.bitdepth), int(fh.frame_data_type)
        else:
            import arm_layouts as al

            c = al.make_case(next(s for s in al.specs() if s[0] == name))
            self.hdr, self.nn, payload, self.bitdepth, self.fdt = c.hdr, c.nn, None, 8, 0
        self.name = name
        dec = DecodeBatch(0)
        if payload is not None:
            dec.add(self.hdr, self.nn, payload, self.bitdepth, self.fdt)
        else:  # the latents the case was written from (its ARM may be one that only the generic entropy kernel's LDS cannot hold)
            dec.add_latents(writer.parse_cc_header(self.hdr), self.nn, c.latents, self.bitdepth, self.fdt)
        dec.run(); dec.wait()
        self.arch = dec.header(0)
        self.host_latents = [dec.latent(0, g) for g in range(self.arch.n_grids)] if payload is not None else c.latents
        self.latents = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in self.host_latents]
        self.ptrs = [t.data_ptr() for t in self.latents]
        self.own_planes = dec.planes(0)
        dec.close()
        rng = np.random.default_rng(len(name))
        maxv = 2 ** self.bitdepth - 1
        self.source_planes = [np.clip(p.astype(np.int64) + rng.integers(-3, 4, p.shape), 0, maxv).astype(p.dtype) for p in self.own_planes]
        self.fdt_name = ["rgb", "yuv420", "yuv444"][self.fdt]
        self.source = _planes_to_frame_data(self.source_planes, self.bitdepth, self.fdt_name)
        self.ints = writer.network_values(self.arch, self.nn)
        self.floats = writer.dequantise_network(self.arch, self.ints)
        self._searches = {}

    def search(self, lmbda=1e-3, floats=None, key=None, **kw):
        from cool_chic_amd import NetworkQuantiser

        k = (lmbda, key, tuple(sorted(kw.items())))
        if k not in self._searches:
            init = {a: kw.pop(a) for a in ("max_in_flight_bytes",) if a in kw}
            self._searches[k] = NetworkQuantiser(0, **init).search(self.arch, self.floats if floats is None else floats, self.ptrs, self.source,
                                                                    lmbda, owner=self.latents, **kw)
        return self._searches[k]

    def alone(self, header, bytes_nn, lmbda):
        from cool_chic_amd import RdEvaluator

        with RdEvaluator(0) as ev:
            ev.add(header, bytes_nn, self.ptrs, self.source, owner=self.latents)
            return ev.evaluate(lmbda)[0]


_CASES = {}


@pytest.fixture
def case(gpu, oracle):
    def get(name):
        if name not in _CASES:
            _CASES[name] = _Case(gpu, oracle, name)
        return _CASES[name]
    return get


def _replay(tables):
    """[(table, steps before the module was visited)]: what the other modules were held at."""
    from cool_chic_amd.nnquant import MODULES

    steps = [f for _, f in TABLES]
    out = []
    for t in tables:
        out.append((t, list(steps)))
        if t.chosen is not None:
            _, gw, gb = next(m for m in MODULES if m[0] == t.module)
            steps[gw], steps[gb] = t.cells[t.chosen].q_w, t.cells[t.chosen].q_b
    return out, steps


def _rank(cells):
    ranked = sorted((c.cost, c.n_bytes_nn, -c.q_w, -c.q_b, i) for i, c in enumerate(cells) if c.feasible)
    return ranked[0][4] if ranked else None


@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_CASES)
def test_meter_shortcuts_are_exact(case, name):
    """Every checked cell of every table equals RdEvaluator.evaluate of that candidate added alone: skipping the meter that a
    module cannot change loses nothing, and neither does sharing a launch with hundreds of other candidates."""
    from cool_chic_amd.nnquant import MODULES, build_network

    c = case(name)
    lmbda = 1e-3
    res = c.search(lmbda)
    has_ifce = c.arch.output_feature_ifce > 0
    assert has_ifce == (name != NO_IFCE_CASE) and [t.module for t in res.tables] == [m[0] for m in MODULES if has_ifce or m[0] != "ifce"]
    rng = np.random.default_rng(6)
    checked = 0
    for t, steps in _replay(res.tables)[0]:
        n = len(t.cells)
        _, gw, gb = next(m for m in MODULES if m[0] == t.module)
        nb = TABLES[gb][0]
        which = list(range(n)) if t.module == "upsampling" else sorted({0, nb - 1, n - nb, n - 1} | set(rng.choice(n, 24, replace=False).tolist()))
        assert len(which) >= (13 if t.module == "upsampling" else 24)
        for i in which:
            cell = t.cells[i]
            s = list(steps)
            s[gw], s[gb] = cell.q_w, cell.q_b
            net = build_network(c.arch, c.floats, s)
            assert net is not None and net.feasible and cell.feasible, (t.module, i)
            want = c.alone(net.header, net.bytes_nn, lmbda)
            assert cell.n_bytes_nn == len(net.bytes_nn) == want.rate.n_bytes_nn
            assert _u64([cell.mse, cell.bits, cell.cost]) == _u64([want.mse, want.bits, want.cost]), (t.module, cell.q_w, cell.q_b)
            checked += 1
    assert checked >= 13 + 2 * 24
    assert _u64([res.candidate.mse, res.candidate.bits, res.candidate.cost]) == _u64(list(res.tables[-1].cells[res.tables[-1].chosen][4:7]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_CASES)
def test_tables_are_complete_and_the_choice_is_their_minimum(case, name):
    from cool_chic_amd.nnquant import module_cells

    c = case(name)
    res = c.search(1e-3)
    sizes = {"arm": 153, "ifce": 153, "upsampling": 13, "synthesis": 325}
    replayed, steps = _replay(res.tables)
    for m, (t, _) in zip([0, 1, 2, 3] if c.arch.output_feature_ifce > 0 else [0, 2, 3], replayed):
        assert len(t.cells) == sizes[t.module] and [(x.q_w, x.q_b) for x in t.cells] == module_cells(m)
        assert t.chosen == _rank(t.cells) and t.cells[t.chosen].feasible
        assert all(np.isfinite([x.mse, x.bits, x.cost]).all() for x in t.cells if x.feasible)
    assert list(res.header.nn_q_step_log2) == steps
    assert res.header.nn_n_bytes == len(res.bytes_nn) <= 16383


@pytest.mark.gpu
def test_an_infeasible_cell_is_recorded_and_never_chosen(case):
    """Dense ARM weights (the layout case's own are nearly all zero: seeded normal ones take their place) scaled until the network
    at the finest steps no longer fits the header's 14-bit nn_n_bytes: those cells are in the table as infeasible with their
    size, the choice is a feasible one, and the result is what RdEvaluator makes of it alone."""
    from cool_chic_amd import writer
    from cool_chic_amd.nnquant import build_network

    c = case(FAT_ARM_CASE)
    layout = writer.network_layout(c.arch)
    assert layout[0] >= 8000
    finest = [f for _, f in TABLES]
    x = c.floats.copy()
    x[:layout[0]] = (np.random.default_rng(7).standard_normal(layout[0]) / 64.0).astype(np.float32)
    for _ in range(16):
        net = build_network(c.arch, x, finest)
        if net is not None and len(net.bytes_nn) > 16383:
            break
        x[:layout[0]] *= 2.0
    assert net is not None and not net.feasible and len(net.bytes_nn) > 16383
    res = c.search(1e-3, floats=x, key="scaled")
    arm = res.tables[0]
    assert arm.module == "arm" and len(arm.cells) == 153
    bad = [i for i, cell in enumerate(arm.cells) if not cell.feasible]
    assert 0 in bad and len(bad) < 153 and all(arm.cells[i].n_bytes_nn > 16383 and np.isnan(arm.cells[i].cost) for i in bad)
    assert all(arm.cells[i].q_w == finest[0] for i in bad) and len(bad) >= 8  # the finest weight step, with all but the coarsest bias steps
    assert all(cell.n_bytes_nn <= 16383 for cell in arm.cells if cell.feasible)
    assert arm.chosen == _rank(arm.cells) and arm.chosen not in bad
    for t in res.tables:
        assert t.chosen is not None and t.cells[t.chosen].feasible and t.cells[t.chosen].n_bytes_nn <= 16383
    assert len(res.bytes_nn) <= 16383 and res.header.nn_n_bytes == len(res.bytes_nn)
    want = c.alone(res.header, res.bytes_nn, 1e-3)
    assert _u64([res.candidate.cost]) == _u64([want.cost]) == _u64([res.tables[-1].cells[res.tables[-1].chosen].cost])


@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_CASES)
def test_the_fixtures_own_steps(case, name):
    from cool_chic_amd import writer
    from cool_chic_amd.nnquant import build_network

    c = case(name)
    own_steps = list(c.arch.nn_q_step_log2)
    own = build_network(c.arch, c.floats, own_steps)
    assert own is not None and own.feasible and np.array_equal(own.values, c.ints) and len(own.bytes_nn) <= len(c.nn)
    for lmbda in (0.0, 1e-4, 1e-2):
        res = c.search(lmbda)
        fixture = c.alone(c.arch, c.nn, lmbda)
        print(f"{name} lambda {lmbda}: fixture cost {fixture.cost!r} ({len(c.nn)} bytes of networks), searched {res.candidate.cost!r} "
              f"({len(res.bytes_nn)} bytes, steps {list(res.header.nn_q_step_log2)}, the fixture's {own_steps})")
        # the table cell at the fixture's own steps, where the other modules stood at the fixture's steps too, is the fixture's network
        for t, steps in _replay(res.tables)[0]:
            gw = {"arm": 0, "ifce": 2, "upsampling": 4, "synthesis": 6}[t.module]
            s = list(steps)
            s[gw], s[gw + 1] = own_steps[gw], own_steps[gw + 1]
            cell = next(x for x in t.cells if (x.q_w, x.q_b) == (own_steps[gw], own_steps[gw + 1]))
            net = build_network(c.arch, c.floats, s)
            at = np.cumsum([0] + writer.network_layout(c.arch))
            assert cell.feasible and cell.n_bytes_nn == len(net.bytes_nn) and np.array_equal(net.values[at[gw]:at[gw + 2]], c.ints[at[gw]:at[gw + 2]])
        assert res.candidate.cost <= fixture.cost, (name, lmbda)


@pytest.mark.gpu
def test_sweeps_and_chunking(case):
    from cool_chic_amd import NetworkQuantiser

    c = case("odd18x65")
    res = c.search(1e-3, sweeps=3)
    n_mod = 4
    assert len(res.tables) % n_mod == 0 and n_mod < len(res.tables) <= 3 * n_mod
    per_sweep = [res.tables[k + n_mod - 1] for k in range(0, len(res.tables), n_mod)]
    costs = [t.cells[t.chosen].cost for t in per_sweep]
    assert all(b <= a for a, b in zip(costs, costs[1:])), costs
    chosen = [[(t.cells[t.chosen].q_w, t.cells[t.chosen].q_b) for t in res.tables[k:k + n_mod]] for k in range(0, len(res.tables), n_mod)]
    # the search stopped after the first sweep that changed nothing, or at the limit
    assert all(a != b for a, b in zip(chosen[:-2], chosen[1:-1]))
    assert len(chosen) == 3 or chosen[-1] == chosen[-2]
    within = [t.cells[t.chosen].cost for t in res.tables]
    assert all(b <= a for a, b in zip(within, within[1:]))  # nor does it rise from module to module
    # chunks of 1, of 7 and of everything: the same tables, bit for bit
    one = c.search(1e-3)
    sb = max(NetworkQuantiser.slot_bytes(c.arch, m) for m in range(4))
    for budget, want_chunk in ((1, 1), (7 * sb + sb // 2, 7)):
        other = c.search(1e-3, max_in_flight_bytes=budget)
        assert min(h.chunk for h in other.pricing) == want_chunk and min(h.chunk for h in one.pricing) >= 325
        assert len(other.pricing) == len(other.tables) and all(0.0 <= h.build_seconds <= h.seconds for h in other.pricing)
        assert other.bytes_nn == one.bytes_nn and bytes(other.header) == bytes(one.header)
        for a, b in zip(other.tables, one.tables):
            assert a.chosen == b.chosen and len(a.cells) == len(b.cells)
            for x, y in zip(a.cells, b.cells):
                assert x[:4] == y[:4] and _u64(list(x[4:])) == _u64(list(y[4:]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rgb192", IFCE_CASE, NO_IFCE_CASE])
def test_fast_path_only(case, name):
    from cool_chic_amd import writer

    c = case(name)
    free = c.search(1e-3)
    fast = c.search(1e-3, fast_path_only=True)
    assert writer.fits_fast_path(writer.cc_header_bytes(fast.header), fast.bytes_nn)
    assert fast.candidate.cost >= free.candidate.cost
    for t in fast.tables:
        for cell in t.cells:
            assert cell.feasible or np.isnan(cell.cost)
    print(f"{name}: unrestricted {free.candidate.cost!r}, fast path only {fast.candidate.cost!r}, "
          f"infeasible cells {[sum(not x.feasible for x in t.cells) for t in fast.tables]}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_CASES)
def test_end_to_end_through_the_oracle(case, oracle, name):
    from cool_chic_amd import DecodeBatch, writer

    c = case(name)
    res = c.search(1e-3)
    stream = writer.encode_stream(writer.cc_header_bytes(res.header), res.bytes_nn, c.host_latents, bitdepth=c.bitdepth, frame_data_type=c.fdt)
    frame, = oracle.decode_video(stream)
    sse = [int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum()) for a, b in zip(frame["planes"], c.source_planes)]
    assert sse == list(res.candidate.quality.sse) and [p.size for p in frame["planes"]] == list(res.candidate.quality.n)
    (_, ccs), = oracle.split_stream(stream)[1]
    hdr, nn, payload = ccs[0]
    parsed = oracle.read_cc_header(hdr)[0]
    assert parsed.nn_n_bytes == len(res.bytes_nn) == res.header.nn_n_bytes == res.candidate.rate.n_bytes_nn and nn == res.bytes_nn
    h2 = writer.parse_cc_header(hdr)
    assert list(h2.nn_q_step_log2) == list(res.header.nn_q_step_log2) and list(h2.nn_expgol_cnt) == list(res.header.nn_expgol_cnt)
    assert h2.nn_n_bit_pad == res.header.nn_n_bit_pad
    assert np.array_equal(oracle.decode_coolchic(hdr, nn, payload, stop_after_entropy=True)["nn_ints"], res.values)
    dec = DecodeBatch(0)
    dec.add(hdr, nn, payload, c.bitdepth, c.fdt)
    dec.run(); dec.wait()
    assert all(np.array_equal(a, b) for a, b in zip(dec.planes(0), frame["planes"]))
    dec.close()


@pytest.mark.gpu
def test_the_tool(gpu, oracle, tmp_path):
    """tools/quantise_networks.py on odd100x37 in a child process: exit 0, and the stream it wrote decodes (the oracle)."""
    name = "odd100x37"
    bs = load_golden(name)[0]
    planes = oracle.decode_video(bs)[0]["planes"]
    rng = np.random.default_rng(12)
    noisy = [np.clip(p.astype(np.int64) + rng.integers(-3, 4, p.shape), 0, 255).astype(np.uint8) for p in planes]
    src, inp, out = tmp_path / "source.ppm", tmp_path / "in.cool", tmp_path / "out.cool"
    h, w = noisy[0].shape
    src.write_bytes(b"P6 %d %d 255\n" % (w, h) + np.stack(noisy, axis=-1).tobytes())
    inp.write_bytes(bs)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "quantise_networks.py"), str(inp), str(src), str(out), "--lmbda", "1e-3",
                        "--sweeps", "2", "--descend", "2"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0
    assert "searched:" in r.stdout and "descended:" in r.stdout
    back = oracle.decode_video(out.read_bytes())
    assert len(back) == 1 and [p.shape for p in back[0]["planes"]] == [p.shape for p in planes]
    (_, ccs), = oracle.split_stream(out.read_bytes())[1]
    assert 0 < len(ccs[0][1]) <= 16383
