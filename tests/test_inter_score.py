"""InterScore / ccd_iscore_* (DESIGN.md section 4.19): the squared error of many candidates of P / B frames per launch.

CPU: the entry points are declared, exported and bound; every refusal comes back from a handle on device -1, that is, before the
device is touched, and a valid call gets as far as CCD_ERR_HIP.
GPU: the yardstick is existing code only - ccd_inter_reconstruct, then QualityMeter.score_planes - over random float outputs,
reference and source planes; every sse[p] and n[p] is compared as an integer.  The inputs are those tests/test_inter_reconstruct.py
feeds the reconstruction (its flow classes, the non-finite ones included, here in both outputs)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from test_inter_reconstruct import case_data

ERR_VALUE, ERR_HIP, ERR_ARG = -2, -6, -7
ENTRY_POINTS = ["ccd_iscore_create", "ccd_iscore_destroy", "ccd_iscore_add_frame", "ccd_iscore_add", "ccd_iscore_clear_items",
                "ccd_iscore_run", "ccd_iscore_wait", "ccd_iscore_frame_result", "ccd_iscore_result"]


# ---- CPU -------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    import cool_chic_amd
    from cool_chic_amd import _lib

    with open(os.path.join(ROOT, "include", "ccd.h")) as f:
        header = f.read()
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert name + "(" in header and name in _lib.SIGNATURES and getattr(L, name) is not None, name
    assert "ccd_iscore_api.cpp" in cool_chic_amd._build.SOURCES
    assert cool_chic_amd.InterScore.__name__ == "InterScore"
    assert all(hasattr(cool_chic_amd.InterScore, m) for m in ("add_frame", "add", "clear_items", "run", "wait", "frame_sse", "sse"))


def test_refusals_come_before_the_device():
    """A handle on device -1: whatever passes the checks fails in hipSetDevice(-1), so a refusal with another code was decided
    before the device was touched.  The host buffers below are never read."""
    from cool_chic_amd._lib import IScoreFrame, lib

    L = lib()
    assert L.ccd_iscore_create(-1, None) == ERR_ARG
    h = C.c_void_p()
    assert L.ccd_iscore_create(-1, C.byref(h)) == 0 and h.value
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data

    def frame(**kw):
        a = dict(frame_type=1, h=8, w=10, bitdepth=10, fdt=1, taps=8, residue=p, motion=p, ref0=(p, p, p), ref1=(None, None, None),
                 src=(p, p, p))
        a.update(kw)
        return IScoreFrame(frame_type=a["frame_type"], h=a["h"], w=a["w"], bitdepth=a["bitdepth"], frame_data_type=a["fdt"],
                           residue=a["residue"], motion=a["motion"], ref0=(C.c_void_p * 3)(*a["ref0"]), ref1=(C.c_void_p * 3)(*a["ref1"]),
                           src=(C.c_void_p * 3)(*a["src"]), global_flow=(C.c_int32 * 4)(1, -1, 0, 0), warp_filter_size=a["taps"])

    def add_frame(**kw):
        return L.ccd_iscore_add_frame(h, C.byref(frame(**kw)))

    def valid_calls_reach_the_device():
        assert add_frame() == ERR_HIP, "a valid call must get as far as hipSetDevice(-1)"
        assert add_frame(frame_type=2, ref1=(p, p, p)) == ERR_HIP
        assert add_frame(fdt=0, h=7, w=9) == ERR_HIP and add_frame(fdt=2, h=1, w=16383) == ERR_HIP  # odd sides outside 4:2:0
        for taps in (2, 4, 6, 16):
            assert add_frame(taps=taps) == ERR_HIP

    valid_calls_reach_the_device()
    assert L.ccd_iscore_add_frame(None, C.byref(frame())) == ERR_ARG and L.ccd_iscore_add_frame(h, None) == ERR_ARG
    arg = [dict(residue=None), dict(motion=None), dict(ref0=(p, None, p)), dict(ref0=(None, p, p)), dict(src=(p, p, None)),
           dict(frame_type=2), dict(frame_type=2, ref1=(p, p, None)),  # ref1 missing for a B frame
           dict(frame_type=0), dict(frame_type=3), dict(bitdepth=7), dict(bitdepth=17), dict(fdt=-1), dict(fdt=3)]
    for kw in arg:
        assert add_frame(**kw) == ERR_ARG, kw
    value = [dict(taps=0), dict(taps=1), dict(taps=3), dict(taps=18), dict(h=7), dict(w=9), dict(h=7, w=9),  # yuv420, odd sides
             dict(fdt=0, h=0), dict(fdt=0, w=0), dict(fdt=0, h=-4), dict(fdt=0, h=16384), dict(fdt=2, w=16384)]
    for kw in value:
        assert add_frame(**kw) == ERR_VALUE, kw
    # items, results and indices: the handle holds no frame, every index is out of range
    assert L.ccd_iscore_add(None, 0, 0, p) == ERR_ARG and L.ccd_iscore_add(h, 0, 0, None) == ERR_ARG
    for frame_index, role in ((0, -1), (0, 2), (-1, 0), (0, 0), (1, 1)):
        assert L.ccd_iscore_add(h, frame_index, role, p) == ERR_ARG, (frame_index, role)
    sse, n = (C.c_uint64 * 3)(7, 7, 7), (C.c_uint64 * 3)(7, 7, 7)
    for fn in (L.ccd_iscore_frame_result, L.ccd_iscore_result):
        assert fn(None, 0, sse, n) == ERR_ARG and fn(h, 0, None, n) == ERR_ARG and fn(h, 0, sse, None) == ERR_ARG
        assert fn(h, -1, sse, n) == ERR_ARG and fn(h, 0, sse, n) == ERR_ARG
    assert list(sse) == [7, 7, 7] and list(n) == [7, 7, 7]
    assert L.ccd_iscore_clear_items(None) == ERR_ARG and L.ccd_iscore_run(None, None) == ERR_ARG and L.ccd_iscore_wait(None, None) == ERR_ARG
    assert L.ccd_iscore_clear_items(h) == 0
    # a refused call leaves the handle as it was: still no frame, and what was valid still is
    assert L.ccd_iscore_add(h, 0, 0, p) == ERR_ARG
    valid_calls_reach_the_device()
    L.ccd_iscore_destroy(h)
    L.ccd_iscore_destroy(None)


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cool_chic_amd import InterScore, _lib

    _lib.lib()
    return InterScore


NONFINITE = np.array([np.inf, -np.inf, np.nan, 3e9], dtype=np.float32)


class _Frame:
    """Random inputs of one P / B frame on the device: the base pair, the references, the source; outputs() makes candidates."""

    def __init__(self, frame_type, h, w, fdt, bitdepth, taps, flow, gflow, seed):
        import torch

        self.ft, self.h, self.w, self.fdt, self.bd, self.taps, self.flow, self.gflow = frame_type, h, w, fdt, bitdepth, taps, flow, list(gflow)
        self.id = f"{'PB'[frame_type - 1]}-{h}x{w}-{('rgb', 'yuv420', 'yuv444')[fdt]}-{bitdepth}bit-n{taps}-{flow}"
        self.seed = seed = [int(v) for v in seed]
        self.dt = torch.uint8 if bitdepth == 8 else torch.uint16
        self.n_refs = 2 if frame_type == 2 else 1
        res, mot, r0, r1 = case_data(dict(seed=seed, h=h, w=w, frame_type=frame_type, bitdepth=bitdepth, fdt=fdt, flow=flow))
        rng = np.random.default_rng(seed + [5])
        self.residue, self.motion = self._dev(self._spoil(res, rng)), self._dev(mot)
        self.refs = [self._planes(r0)] + ([self._planes(r1)] if r1 is not None else [])
        self.src = self._planes([rng.integers(0, 2 ** bitdepth, size=p.shape) for p in r0])
        self.n = tuple(int(p.numel()) for p in self.src)

    def _spoil(self, res, rng):
        """The non-finite class has its values in the residue output too, colours and blend weights alike."""
        if self.flow != "nonfinite":
            return res
        bad = rng.random(res.shape) < 0.08
        return np.where(bad, rng.choice(NONFINITE, size=res.shape), res).astype(np.float32)

    @staticmethod
    def _dev(a):
        import torch

        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda().contiguous()

    def _planes(self, ps):
        import torch

        return [torch.from_numpy(np.asarray(p).astype(np.int32)).cuda().to(self.dt).contiguous() for p in ps]

    def outputs(self, role, k):
        """Candidate number k of a role: another random output of the frame's flow class."""
        rng = np.random.default_rng(self.seed + [11, role, k])
        res, mot, _, _ = case_data(dict(seed=self.seed + [13, role, k], h=self.h, w=self.w, frame_type=self.ft, bitdepth=self.bd,
                                        fdt=self.fdt, flow=self.flow))
        return self._dev(self._spoil(res, rng) if role == 0 else mot)

    def add_to(self, score):
        return score.add_frame(self.ft, self.h, self.w, self.bd, self.fdt, self.residue.data_ptr(), self.motion.data_ptr(),
                               [p.data_ptr() for p in self.refs[0]], [p.data_ptr() for p in self.refs[1]] if self.ft == 2 else None,
                               [p.data_ptr() for p in self.src], self.gflow, self.taps, owner=self)

    def reconstruct(self, residue, motion):
        """The yardstick's first half: ccd_inter_reconstruct into new planes."""
        import torch

        from cool_chic_amd._lib import check, lib

        out = [torch.zeros_like(p) for p in self.src]

        def ptrs(ps):
            return (C.c_void_p * 3)(*[p.data_ptr() for p in ps])

        st = torch.cuda.current_stream().cuda_stream
        check(lib().ccd_inter_reconstruct(0, C.c_void_p(st or None), self.ft, self.h, self.w, self.bd, self.fdt, C.c_void_p(residue.data_ptr()),
                                          C.c_void_p(motion.data_ptr()), ptrs(self.refs[0]), ptrs(self.refs[1]) if self.ft == 2 else None,
                                          (C.c_int32 * 4)(*self.gflow), self.taps, ptrs(out)), "ccd_inter_reconstruct")
        return out


def _yardstick(jobs):
    """jobs: [(frame, residue, motion)] -> [(sse[3], n[3])] from ccd_inter_reconstruct and QualityMeter.score_planes."""
    from cool_chic_amd.quality import QualityMeter

    planes = [f.reconstruct(r, m) for f, r, m in jobs]
    with QualityMeter(0) as meter:
        q = meter.score_planes(planes, [f.src for f, _, _ in jobs], [f.bd for f, _, _ in jobs], ms_ssim=False)
    return [(tuple(int(v) for v in r.sse), tuple(int(v) for v in r.n)) for r in q]


# (h, w, formats): 2 x 2 one quad; one-pixel sides (no 4:2:0, and the grid_sample warps divide by (n - 1) / 2: sinc sizes only);
# 6 x 70 crosses a 64 x 4 tile on both axes with partial tiles, in units of samples and of quads; the two ragged pictures
SHAPES = [(2, 2, (0, 1, 2)), (1, 1, (0, 2)), (1, 67, (0, 2)), (6, 70, (0, 1, 2)), (38, 130, (1,)), (37, 131, (0,))]
FLOWS = ["subpixel", "beyond_picture", "nonfinite"]
TAPS = [2, 4, 6, 8, 16]


def _matrix(taps):
    """Every shape and format x P / B x 8, 10, 16 bits x every flow class at one filter size, global flows never all zero."""
    frames = []
    for si, (h, w, fmts) in enumerate(SHAPES):
        if taps < 6 and min(h, w) == 1:
            continue
        for fdt in fmts:
            for ft in (1, 2):
                for bi, bd in enumerate((8, 10, 16)):
                    for fi, flow in enumerate(FLOWS):
                        k = len(frames)
                        gflow = [[1, -2, -3, 1], [w + 5, -(h + 7), -(w + 9), h + 3], [-2, 1, 2, -1]][k % 3]
                        frames.append(_Frame(ft, h, w, fdt, bd, taps, flow, gflow, seed=[taps, si, fdt, ft, bi, fi]))
    return frames


@pytest.mark.gpu
@pytest.mark.parametrize("taps", TAPS)
def test_scores_equal_reconstruct_then_quality_meter(gpu, taps):
    """One handle per filter size holds every frame of the matrix with a residue and a motion candidate each: the base pair (mode
    0), the residue item (mode 1, the kept warps) and the motion item (mode 2) all equal the yardstick, sse and n, as integers."""
    frames = _matrix(taps)
    assert {f.ft for f in frames} == {1, 2} and {f.bd for f in frames} == {8, 10, 16} and {f.flow for f in frames} == set(FLOWS)
    assert all(any(f.gflow) for f in frames)
    jobs, cands = [], []
    with gpu(0) as score:
        for f in frames:
            k = f.add_to(score)
            res, mot = f.outputs(0, 0), f.outputs(1, 0)
            cands.append((score.add(k, 0, res.data_ptr(), owner=res), score.add(k, 1, mot.data_ptr(), owner=mot)))
            jobs += [(f, f.residue, f.motion), (f, res, f.motion), (f, f.residue, mot)]
        score.run()
        score.wait()
        got = []
        for k, (i_res, i_mot) in enumerate(cands):
            got += [score.frame_sse(k), score.sse(i_res), score.sse(i_mot)]
    want = _yardstick(jobs)
    bad = [(f.id, "base residue motion".split()[i % 3], g, w) for i, ((f, _, _), g, w) in enumerate(zip(jobs, got, want)) if g != w]
    assert not bad, f"{len(bad)} of {len(jobs)} results differ from the yardstick: {bad[:6]}"
    assert all(w[1] == f.n for (f, _, _), w in zip(jobs, want))


def _two_frames():
    """Different sizes and formats, a sinc-8 B frame and a 4-tap P frame: both kernel instantiations, two launches per stage."""
    return [_Frame(2, 38, 130, 1, 8, 8, "subpixel", [1, -2, -3, 1], seed=[77, 0]),
            _Frame(1, 37, 131, 0, 10, 4, "beyond_picture", [-2, 1, 0, 0], seed=[77, 1])]


def _seventy(frames):
    """70 items over the two frames, roles mixed: [(frame index, role, output)]."""
    rng = np.random.default_rng(70)
    return [(int(k), int(r), frames[int(k)].outputs(int(r), i)) for i, (k, r) in enumerate(zip(rng.integers(0, 2, 70), rng.integers(0, 2, 70)))]


def _job(frames, k, role, out):
    f = frames[k]
    return (f, out, f.motion) if role == 0 else (f, f.residue, out)


@pytest.mark.gpu
def test_one_handle_two_frames_seventy_items(gpu):
    """The prefix table, the per-job partial ranges and the two-launch split: every item of the full handle equals the yardstick
    and the result of a handle that holds it alone; clear_items followed by other items gives those items' values."""
    frames = _two_frames()
    items = _seventy(frames)
    assert {(k, r) for k, r, _ in items} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    want = _yardstick([(f, f.residue, f.motion) for f in frames] + [_job(frames, k, r, o) for k, r, o in items])
    with gpu(0) as score:
        for f in frames:
            f.add_to(score)
        ids = [score.add(k, r, o.data_ptr(), owner=o) for k, r, o in items]
        assert ids == list(range(70))
        score.run()
        score.wait()
        assert [score.frame_sse(k) for k in range(2)] == want[:2]
        got = [score.sse(i) for i in ids]
        assert got == want[2:]
        # other items after clear_items: the last 9 in reverse order
        score.clear_items()
        with pytest.raises(Exception):
            score.sse(0)
        again = items[:-10:-1]
        ids = [score.add(k, r, o.data_ptr(), owner=o) for k, r, o in again]
        assert ids == list(range(9))
        score.run()
        score.wait()
        assert [score.sse(i) for i in ids] == want[2:][:-10:-1]
        assert [score.frame_sse(k) for k in range(2)] == want[:2]
    for i in (0, 1, 2, 3, 33, 69):  # alone: one frame, one item
        k, r, o = items[i]
        with gpu(0) as solo:
            frames[k].add_to(solo)
            solo.add(0, r, o.data_ptr(), owner=o)
            solo.run()
            solo.wait()
            assert solo.sse(0) == want[2 + i], i
            assert solo.frame_sse(0) == want[k]


@pytest.mark.gpu
def test_modes_agree_and_rewritten_buffers_are_followed(gpu):
    """A residue item whose output is the base residue and a motion item whose output is the base motion equal the frame's
    result (mode 1 = mode 2 = mode 0); rewriting the base motion buffer between two runs is followed by the base pair and by the
    residue items, whose kept warps are made again at every run."""
    frames = _two_frames()
    with gpu(0) as score:
        idx = []
        for k, f in enumerate(frames):
            f.add_to(score)
            other = f.outputs(0, 3)
            idx.append((score.add(k, 0, f.residue.data_ptr()), score.add(k, 1, f.motion.data_ptr()), score.add(k, 0, other.data_ptr(), owner=other), other))
        score.run()
        score.wait()
        want = _yardstick([(f, f.residue, f.motion) for f in frames] + [(f, idx[k][3], f.motion) for k, f in enumerate(frames)])
        for k in range(2):
            assert score.frame_sse(k) == want[k] and score.sse(idx[k][0]) == want[k] and score.sse(idx[k][1]) == want[k]
            assert score.sse(idx[k][2]) == want[2 + k]
        first = [score.frame_sse(k) for k in range(2)]
        for f in frames:
            f.motion.copy_(f.outputs(1, 5))
        import torch

        torch.cuda.synchronize()
        score.run()
        score.wait()
        want = _yardstick([(f, f.residue, f.motion) for f in frames] + [(f, idx[k][3], f.motion) for k, f in enumerate(frames)])
        for k in range(2):
            assert score.frame_sse(k) == want[k] != first[k]
            assert score.sse(idx[k][0]) == want[k] and score.sse(idx[k][1]) == want[k] and score.sse(idx[k][2]) == want[2 + k]


@pytest.mark.gpu
def test_a_run_in_flight_refuses_every_change(gpu):
    """Between run() and wait() the handle takes no frame, no item, no clear, no second run and hands out no result
    (CCD_ERR_ARG); after the wait everything works again and the results are the run's."""
    from cool_chic_amd import CcdError

    f = _two_frames()[1]
    out = f.outputs(1, 0)
    with gpu(0) as score:
        f.add_to(score)
        score.add(0, 1, out.data_ptr(), owner=out)
        score.run()
        for call in (lambda: f.add_to(score), lambda: score.add(0, 0, f.residue.data_ptr()), score.clear_items, score.run,
                     lambda: score.frame_sse(0), lambda: score.sse(0)):
            with pytest.raises(CcdError) as e:
                call()
            assert e.value.code == ERR_ARG
        score.wait()
        assert [score.frame_sse(0), score.sse(0)] == _yardstick([(f, f.residue, f.motion), (f, f.residue, out)])
        with pytest.raises(CcdError):
            score.sse(1)
        with pytest.raises(CcdError):
            score.frame_sse(1)
        assert score.add(0, 0, f.residue.data_ptr()) == 1
