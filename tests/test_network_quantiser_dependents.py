"""NetworkQuantiser.search(dependents=...) and rd.cost_with_dependents: an intra frame's candidate networks
priced through the P / B frames that predict from it.

CPU: cost_with_dependents against its formula in exact rationals; a dependent of another size raises ValueError.
GPU: the I frames of `vid5` (a P and two B frames predict from it, 128 x 224) and `vid3_ldp` (one P frame).  The yardstick is
existing code only: RdEvaluator.evaluate of the candidate added alone gives its own cost and its planes, ccd_inter_reconstruct
(dependent_cases.Dependent.reconstruct) of every dependent against those planes and QualityMeter.score_planes give the dependents'
integers, cost_with_dependents joins them; costs are compared as float64 bit patterns."""
from fractions import Fraction

import numpy as np
import pytest

from test_network_quantiser import _rank, _replay, _u64

VIDEOS = ["vid5", "vid3_ldp"]
LAMBDAS = [1e-4, 1e-3, 1e-2, 1e-1]


# ---- CPU -------------------------------------------------------------------------------------------------------------
def test_cost_with_dependents_is_the_formula():
    from cool_chic_amd.rd import cost_with_dependents, rd_cost

    rng = np.random.default_rng(422)
    for trial in range(50):
        bd = int(rng.choice([8, 10, 16]))
        own = rd_cost([int(v) for v in rng.integers(0, 10 ** 9, 3)], [28672, 7168, 7168], bd, float(rng.integers(1, 10 ** 6)), 400, 30, 28672, 1e-3)
        deps = []
        for _ in range(int(rng.integers(0, 5))):
            d_bd = int(rng.choice([8, 10, 16]))
            deps.append(([int(v) for v in rng.integers(0, 10 ** 12, 3)], [int(v) for v in rng.integers(1, 10 ** 5, 3)], d_bd))
        want = own[2]
        for sse, n, d_bd in deps:  # every term the correctly rounded quotient of exact integers, added in list order
            assert sum(n) * (2 ** d_bd - 1) ** 2 < 2 ** 53
            want = want + float(Fraction(sum(sse), sum(n) * (2 ** d_bd - 1) ** 2))
        got = cost_with_dependents(own, deps)
        assert isinstance(got, float) and _u64([got]) == _u64([want]), trial
    own = (0.25, 100.0, 0.5)
    assert cost_with_dependents(own, []) == 0.5
    assert cost_with_dependents(own, [((255 ** 2, 0, 0), (1, 0, 0), 8)]) == 1.5
    # list order: float64 addition is not associative
    a, b = ((1, 0, 0), (3, 0, 0), 8), ((10 ** 15, 0, 0), (7, 0, 0), 8)
    assert cost_with_dependents(own, [a, b]) == (0.5 + 1 / (3.0 * 65025.0)) + 10 ** 15 / (7.0 * 65025.0)


def test_a_dependent_of_another_size_raises():
    """The dependents are checked before anything else of the search: no device is touched, nothing is decoded."""
    from cool_chic_amd import NetworkQuantiser, nnquant
    from cool_chic_amd._lib import CCHeader
    from cool_chic_amd.quality import _planes_to_frame_data

    def frame(h, w, bd=8, fmt="yuv420"):
        dt = np.uint8 if bd == 8 else np.uint16
        ch, cw = (h // 2, w // 2) if fmt == "yuv420" else (h, w)
        return _planes_to_frame_data([np.zeros((h, w), dt), np.zeros((ch, cw), dt), np.zeros((ch, cw), dt)], bd, fmt)

    src = frame(16, 32)
    arch = CCHeader()
    arch.img_size[0], arch.img_size[1] = 16, 32
    for other in (frame(16, 34), frame(18, 32), frame(16, 32, 10), frame(16, 32, 8, "yuv444")):
        dep = nnquant.Dependent(1, 0, 1, 1, None, (0, 0, 0, 0), 8, other)
        with pytest.raises(ValueError, match="dependent 1"):
            NetworkQuantiser(-1).search(arch, np.zeros(1, np.float32), [], src, 1e-3, dependents=[nnquant.Dependent(1, 0, 1, 1, None, (0, 0, 0, 0), 8, src), dep])
    for bad in (nnquant.Dependent(1, 1, 1, 1, None, (0, 0, 0, 0), 8, src), nnquant.Dependent(2, 0, 1, 1, None, (0, 0, 0, 0), 8, src),
                nnquant.Dependent(3, 0, 1, 1, None, (0, 0, 0, 0), 8, src)):
        with pytest.raises(ValueError, match="dependent 0"):
            NetworkQuantiser(-1).search(arch, np.zeros(1, np.float32), [], src, 1e-3, dependents=[bad])


# ---- GPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cool_chic_amd import _lib

    _lib.lib()
    return torch


class _Video:
    """The I frame (coding index 0) of a video fixture as NetworkQuantiser takes it - latents on the device, the float parameters
    its integers dequantise to, a source of its decoded planes plus seeded noise of `noise` LSB - and its DIRECT dependents."""

    def __init__(self, torch, name, noise=3):
        import dependent_cases as dc
        import inter_cases as ic

        from cool_chic_amd import DecodeBatch, writer
        from cool_chic_amd.nnquant import Dependent
        from cool_chic_amd.quality import _frame_planes, _planes_to_frame_data

        frames = ic.parse_video(name)
        fh, ccs, display, _ = frames[0]
        assert fh.frame_type == 0
        arch, hdr, self.nn, payload = ccs[0]
        self.bd, self.fdt = int(fh.bitdepth), int(fh.frame_data_type)
        self.fdt_name = ic.FDT_NAMES[self.fdt]
        dec = DecodeBatch(0)
        dec.add(hdr, self.nn, payload, self.bd, self.fdt)
        dec.run(); dec.wait()
        self.arch = dec.header(0)
        self.latents = [torch.from_numpy(np.ascontiguousarray(dec.latent(0, g))).cuda() for g in range(self.arch.n_grids)]
        self.ptrs = [t.data_ptr() for t in self.latents]
        own = dec.planes(0)
        dec.close()
        rng = np.random.default_rng([len(name), noise])
        self.source = _planes_to_frame_data([np.clip(p.astype(np.int64) + rng.integers(-noise, noise + 1, p.shape), 0, 2 ** self.bd - 1).astype(p.dtype)
                                             for p in own], self.bd, self.fdt_name)
        self.floats = writer.dequantise_network(self.arch, writer.network_values(self.arch, self.nn))
        self.deps, self.descriptors = [], []
        for k, (dfh, _, _, refs) in enumerate(frames):
            n_refs = int(dfh.frame_type)
            if display not in refs[:n_refs]:
                continue
            c = ic.case(name, k)
            d = dc.Dependent(c, refs[:n_refs].index(display))
            source = _planes_to_frame_data([p.cpu().numpy() for p in c.src], c.bd, ic.FDT_NAMES[c.fdt])
            assert all(torch.equal(a, b) for a, b in zip(_frame_planes(source, torch.device("cuda:0")), c.src))
            other = c.refs[1 - d.which] if c.frame_type == 2 else None
            self.deps.append(d)
            self.descriptors.append(Dependent(c.frame_type, d.which, d.residue.data_ptr(), d.motion.data_ptr(),
                                              None if other is None else [t.data_ptr() for t in other], d.gflow, c.taps, source, owner=(c, d)))
        self._searches = {}

    def search(self, lmbda, dependents=True, source=None, **kw):
        from cool_chic_amd import NetworkQuantiser

        key = (lmbda, dependents, id(source), tuple(sorted(kw.items())))
        if key not in self._searches:
            if dependents is not None:
                kw["dependents"] = self.descriptors if dependents is True else dependents
            self._searches[key] = NetworkQuantiser(0).search(self.arch, self.floats, self.ptrs, source or self.source, lmbda, owner=self.latents, **kw)
        return self._searches[key]

    def yardstick(self, nets, lmbda, source=None):
        """[(own Candidate, [(sse, n, bitdepth)] per dependent)] of (header, bytes_nn) networks: one RdEvaluator over all of them,
        then every dependent reconstructed against every candidate's planes and scored."""
        from cool_chic_amd import RdEvaluator
        from cool_chic_amd.quality import QualityMeter

        with RdEvaluator(0) as ev, QualityMeter(0) as meter:
            for header, bytes_nn in nets:
                ev.add(header, bytes_nn, self.ptrs, source or self.source, owner=self.latents)
            own = ev.evaluate(lmbda)
            terms = [[] for _ in nets]
            for d in self.deps:
                rec = [d.reconstruct(ev.planes(s)) for s in range(len(nets))]
                res = meter.score_planes(rec, [d.src] * len(rec), [d.case.bd] * len(rec), [self.fdt_name] * len(rec), ms_ssim=False)
                for s, r in enumerate(res):
                    terms[s].append((tuple(int(v) for v in r.sse), tuple(int(v) for v in r.n), d.case.bd))
        return list(zip(own, terms))


_VIDEOS = {}


@pytest.fixture
def video(gpu):
    def get(name, **kw):
        key = (name, tuple(sorted(kw.items())))
        if key not in _VIDEOS:
            _VIDEOS[key] = _Video(gpu, name, **kw)
        return _VIDEOS[key]
    return get


def _cell_nets(v, t, steps, which):
    from cool_chic_amd.nnquant import MODULES, build_network

    _, gw, gb = next(m for m in MODULES if m[0] == t.module)
    nets = []
    for i in which:
        s = list(steps)
        s[gw], s[gb] = t.cells[i].q_w, t.cells[i].q_b
        net = build_network(v.arch, v.floats, s)
        assert net is not None and net.feasible and t.cells[i].feasible, (t.module, i)
        nets.append((net.header, net.bytes_nn))
    return nets


@pytest.mark.gpu
@pytest.mark.parametrize("name", VIDEOS)
def test_cells_equal_the_candidate_alone_plus_its_dependents(video, name):
    from cool_chic_amd.nnquant import MODULES, build_network
    from cool_chic_amd.rd import cost_with_dependents

    v = video(name)
    assert [d.case.frame_type for d in v.deps] == ([1, 2, 2] if name == "vid5" else [1])
    lmbda = 1e-3
    res = v.search(lmbda)
    rng = np.random.default_rng(22)
    checked = {"moving": 0, "kept": 0}
    for t, steps in _replay(res.tables)[0]:
        n = len(t.cells)
        which = sorted({t.chosen, 0, n - 1} | set(rng.choice(n, 5, replace=False).tolist()))
        want = v.yardstick(_cell_nets(v, t, steps, which), lmbda)
        if t.module in ("upsampling", "synthesis"):
            for i, (own, terms) in zip(which, want):
                cell = t.cells[i]
                assert _u64([cell.mse, cell.bits]) == _u64([own.mse, own.bits]), (t.module, i)
                assert _u64([cell.cost]) == _u64([cost_with_dependents((own.mse, own.bits, own.cost), terms)]), (t.module, i)
                assert cell.cost > own.cost
                checked["moving"] += 1
        else:  # the planes do not move: the dependent term of the network the other modules are held at
            held = build_network(v.arch, v.floats, steps)
            (_, held_terms), = v.yardstick([(held.header, held.bytes_nn)], lmbda)
            for i, (own, terms) in zip(which, want):
                assert terms == held_terms
                assert _u64([t.cells[i].cost]) == _u64([cost_with_dependents((own.mse, own.bits, own.cost), held_terms)]), (t.module, i)
                checked["kept"] += 1
        assert t.chosen == _rank(t.cells)
    assert checked["moving"] >= 2 * 7 and checked["kept"] >= 7
    (own, terms), = v.yardstick([(res.header, res.bytes_nn)], lmbda)
    assert tuple(res.dependents) == tuple((s, n) for s, n, _ in terms) and len(res.dependents) == len(v.deps)
    assert _u64([res.candidate.cost]) == _u64([own.cost])


@pytest.mark.gpu
def test_without_dependents_nothing_changes(video):
    v = video("vid3_ldp")
    a = v.search(1e-3, dependents=None)
    b = v.search(1e-3, dependents=None, sweeps=1)  # (another cache key: a second search that does not pass the argument either)
    c = v.search(1e-3, dependents=())
    assert a is not b
    for x in (b, c):
        assert bytes(x.bytes_nn) == bytes(a.bytes_nn) and list(x.header.nn_q_step_log2) == list(a.header.nn_q_step_log2)
        assert _u64([x.candidate.mse, x.candidate.bits, x.candidate.cost]) == _u64([a.candidate.mse, a.candidate.bits, a.candidate.cost])
        assert [getattr(x.candidate.rate, f) for f in ("total_bits", "n_bytes_nn", "n_bytes_header")] == \
            [getattr(a.candidate.rate, f) for f in ("total_bits", "n_bytes_nn", "n_bytes_header")]
        assert tuple(x.candidate.quality.sse) == tuple(a.candidate.quality.sse)
        assert [(t.module, t.chosen, [_u64(list(cl[4:7])) for cl in t.cells]) for t in x.tables] == \
            [(t.module, t.chosen, [_u64(list(cl[4:7])) for cl in t.cells]) for t in a.tables]
        assert x.dependents == ()
    assert _replay(a.tables)[1] == list(a.header.nn_q_step_log2)


@pytest.mark.gpu
def test_slot_bytes_counts_the_reference_items(video):
    from cool_chic_amd import NetworkQuantiser

    v = video("vid5")
    px = int(v.arch.img_size[0]) * int(v.arch.img_size[1])
    for m in range(4):
        extra = NetworkQuantiser.slot_bytes(v.arch, m, 3) - NetworkQuantiser.slot_bytes(v.arch, m)
        assert extra == (36 * px if m >= 2 else 0)


# a (fixture, source noise, lambda) at which the dependents change the choice of the synthesis table.  Found by a sweep over both
# fixtures, noise of 1 / 3 / 8 LSB and the four lambdas of LAMBDAS: the choice changes at every lambda for vid5
# and at 1e-4 .. 1e-2 for vid3_ldp; the test itself shows it again with the yardstick alone before it looks at the search.
CHANGING = ("vid5", 3, 1e-3)


@pytest.mark.gpu
def test_the_dependents_change_the_choice(video):
    """By the yardstick alone, over the whole synthesis table at the steps the search held: the argmin with the dependent term
    is another cell than the argmin of the own cost.  Then: the search chose the former."""
    from cool_chic_amd.rd import cost_with_dependents

    name, noise, lmbda = CHANGING
    assert lmbda in LAMBDAS
    v = video(name, noise=noise)
    res = v.search(lmbda)
    (t, steps), = [(t, s) for t, s in _replay(res.tables)[0] if t.module == "synthesis"]
    live = [i for i, c in enumerate(t.cells) if c.feasible]
    want = v.yardstick(_cell_nets(v, t, steps, live), lmbda)

    def argmin(costs):
        return min(zip(live, costs), key=lambda ic: (ic[1], t.cells[ic[0]].n_bytes_nn, -t.cells[ic[0]].q_w, -t.cells[ic[0]].q_b))[0]

    without = argmin([own.cost for own, _ in want])
    with_term = argmin([cost_with_dependents((own.mse, own.bits, own.cost), terms) for own, terms in want])
    assert with_term != without, "the yardstick's two choices are the same cell: the case does not show what it is meant to"
    assert t.chosen == with_term
    assert (t.cells[t.chosen].q_w, t.cells[t.chosen].q_b) == (res.header.nn_q_step_log2[6], res.header.nn_q_step_log2[7])


@pytest.mark.gpu
def test_the_tool_with_dependents(gpu, oracle, tmp_path):
    """tools/quantise_video_networks.py --dependents on vid5 (I P B B B) in a child process: exit 0 (its decode-back assertion
    inside), the I frame reports the summed cost with its three direct dependents before and after, and the written stream decodes."""
    import os
    import subprocess
    import sys

    from conftest import GOLDEN, ROOT

    name = "vid5"
    with open(os.path.join(GOLDEN, name + ".cool"), "rb") as f:
        bs = f.read()
    rng = np.random.default_rng(22)
    decoded = oracle.decode_video(bs)
    yuv, out = tmp_path / "source.yuv", tmp_path / "out.cool"
    with open(yuv, "wb") as f:
        for frame in decoded:  # display order
            for p in frame["planes"]:
                f.write(np.clip(p.astype(np.int64) + rng.integers(-3, 4, p.shape), 0, 255).astype(np.uint8).tobytes())
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "quantise_video_networks.py"), os.path.join(GOLDEN, name + ".cool"), str(yuv),
                        str(out), "--lmbda", "1e-3", "--dependents"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0
    assert r.stdout.count("before:") == 5 and r.stdout.count("after:") == 5
    assert r.stdout.count("with its 3 direct dependents (searched with them): summed cost") == 1
    assert len(oracle.decode_video(out.read_bytes())) == 5
