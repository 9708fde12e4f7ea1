"""InterScore.add_refs / ccd_iscore_add_refs: a P / B frame's base pair scored against OTHER reference planes.

CPU: the entry point is declared, exported and bound; every refusal comes back as CCD_ERR_ARG from a handle on device -1, that is,
before the device is touched.  (Such a handle never holds a frame - ccd_iscore_add_frame fails in hipSetDevice(-1) - so the frame
index of every call here is out of range as well; the refusals one by one, on a handle that holds frames, and the valid call are in
the GPU part.)
GPU: the yardstick is existing code only - ccd_inter_reconstruct with the candidate planes passed as the references, then
QualityMeter.score_planes - and every sse[p] and n[p] is compared as an integer.  Frames, shapes and flow classes are those of
tests/test_inter_score.py."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from test_inter_score import FLOWS, TAPS, _Frame, _matrix, _two_frames, _yardstick

ERR_HIP, ERR_ARG = -6, -7


# ---- CPU -------------------------------------------------------------------------------------------------------------------------
def test_add_refs_is_declared_exported_and_bound():
    import cool_chic_amd
    from cool_chic_amd import _lib

    with open(os.path.join(ROOT, "include", "ccd.h")) as f:
        header = f.read()
    assert "ccd_iscore_add_refs(" in header and "ccd_iscore_add_refs" in _lib.SIGNATURES
    assert getattr(_lib.lib(), "ccd_iscore_add_refs") is not None
    assert hasattr(cool_chic_amd.InterScore, "add_refs")


def _ptrs(*ps):
    return (C.c_void_p * 3)(*ps)


def test_refusals_come_before_the_device():
    from cool_chic_amd._lib import lib

    L = lib()
    h = C.c_void_p()
    assert L.ccd_iscore_create(-1, C.byref(h)) == 0 and h.value
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data
    good, hole = _ptrs(p, p, p), _ptrs(p, None, p)
    assert L.ccd_iscore_add_refs(None, 0, good, None) == ERR_ARG
    for frame in (-1, 0, 1):
        assert L.ccd_iscore_add_refs(h, frame, good, None) == ERR_ARG, frame
    assert L.ccd_iscore_add_refs(h, 0, None, None) == ERR_ARG
    for r0, r1 in ((hole, None), (None, hole), (good, hole), (_ptrs(None, p, p), good), (None, good)):
        assert L.ccd_iscore_add_refs(h, 0, r0, r1) == ERR_ARG
    # the handle is as it was: no item, nothing to run, nothing to report
    sse, n = (C.c_uint64 * 3)(7, 7, 7), (C.c_uint64 * 3)(7, 7, 7)
    assert L.ccd_iscore_result(h, 0, sse, n) == ERR_ARG and list(sse) == [7, 7, 7]
    assert L.ccd_iscore_clear_items(h) == 0 and L.ccd_iscore_run(h, None) == 0
    L.ccd_iscore_destroy(h)


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cool_chic_amd import InterScore, _lib

    _lib.lib()
    return InterScore


KINDS = {"ref0": (0,), "ref1": (1,), "both": (0, 1)}


def _candidate_planes(f, k):
    """Candidate number k of a frame: planes for both references, random integers over the full range of the bit depth."""
    rng = np.random.default_rng(f.seed + [17, k])
    return [f._planes([rng.integers(0, 2 ** f.bd, size=tuple(p.shape)) for p in f.src]) for _ in range(2)]


def _with_refs(f, kind, planes):
    """The frame as the yardstick sees a reference item: `planes[r]` in place of the references of `kind`."""
    g = copy.copy(f)
    g.refs = [planes[r] if r in KINDS[kind] else f.refs[r] for r in range(f.n_refs)]
    return g


def _add(score, k, kind, planes):
    r = [[t.data_ptr() for t in planes[i]] if i in KINDS[kind] else None for i in range(2)]
    return score.add_refs(k, r[0], r[1], owner=planes)


def _kinds(f):
    return ("ref0", "ref1", "both") if f.ft == 2 else ("ref0",)


@pytest.mark.gpu
@pytest.mark.parametrize("taps", TAPS)
def test_reference_items_equal_reconstruct_then_quality_meter(gpu, taps):
    """One handle per filter size holds every frame of the matrix with a ref0 item and, B frames, a ref1 item and one with both."""
    frames = _matrix(taps)
    assert {f.ft for f in frames} == {1, 2} and {f.bd for f in frames} == {8, 10, 16} and {f.flow for f in frames} == set(FLOWS)
    jobs, ids, names = [], [], []
    with gpu(0) as score:
        for f in frames:
            k = f.add_to(score)
            planes = _candidate_planes(f, 0)
            for kind in _kinds(f):
                ids.append(_add(score, k, kind, planes))
                g = _with_refs(f, kind, planes)
                jobs.append((g, f.residue, f.motion))
                names.append((f.id, kind))
        assert ids == list(range(len(ids)))
        score.run()
        score.wait()
        got = [score.sse(i) for i in ids]
        base = [score.frame_sse(k) for k in range(len(frames))]
    want = _yardstick(jobs)
    bad = [(nm, g, w) for nm, g, w in zip(names, got, want) if g != w]
    assert not bad, f"{len(bad)} of {len(jobs)} reference items differ from the yardstick: {bad[:6]}"
    assert all(w[1] == f.n for (f, _, _), w in zip(jobs, want))
    assert base == _yardstick([(f, f.residue, f.motion) for f in frames])  # the base pairs are what they are without the items


@pytest.mark.gpu
def test_own_references_as_items_equal_the_frame(gpu):
    frames = _two_frames() + [_Frame(2, 6, 70, 2, 16, 6, "nonfinite", [-2, 1, 2, -1], seed=[78, 0])]
    with gpu(0) as score:
        ids = []
        for k, f in enumerate(frames):
            f.add_to(score)
            ids.append([_add(score, k, kind, f.refs + f.refs[:1]) for kind in _kinds(f)])
        score.run()
        score.wait()
        for k, f in enumerate(frames):
            assert len(ids[k]) == (3 if f.ft == 2 else 1)
            for i in ids[k]:
                assert score.sse(i) == score.frame_sse(k), (f.id, i)
        assert [score.frame_sse(k) for k in range(len(frames))] == _yardstick([(f, f.residue, f.motion) for f in frames])


def _seventy(frames):
    """70 items over the two frames in random order: [(frame index, kind, payload)] - roles 0 / 1 (a float output) and the
    reference kinds the frame has (candidate planes)."""
    rng = np.random.default_rng(71)
    items = []
    for i in range(70):
        k = int(rng.integers(0, 2))
        kinds = (0, 1) + _kinds(frames[k])
        kind = kinds[int(rng.integers(0, len(kinds)))]
        items.append((k, kind, frames[k].outputs(kind, i) if kind in (0, 1) else _candidate_planes(frames[k], i)))
    return items


def _job(frames, k, kind, payload):
    f = frames[k]
    if kind == 0:
        return (f, payload, f.motion)
    if kind == 1:
        return (f, f.residue, payload)
    return (_with_refs(f, kind, payload), f.residue, f.motion)


def _add_item(score, k, kind, payload):
    return score.add(k, kind, payload.data_ptr(), owner=payload) if kind in (0, 1) else _add(score, k, kind, payload)


@pytest.mark.gpu
def test_one_handle_two_frames_seventy_mixed_items(gpu):
    frames = _two_frames()
    items = _seventy(frames)
    assert {(k, kind) for k, kind, _ in items} == {(0, 0), (0, 1), (0, "ref0"), (0, "ref1"), (0, "both"), (1, 0), (1, 1), (1, "ref0")}
    want = _yardstick([(f, f.residue, f.motion) for f in frames] + [_job(frames, *it) for it in items])
    with gpu(0) as score:
        for f in frames:
            f.add_to(score)
        ids = [_add_item(score, *it) for it in items]
        assert ids == list(range(70))
        score.run()
        score.wait()
        assert [score.frame_sse(k) for k in range(2)] == want[:2]
        assert [score.sse(i) for i in ids] == want[2:]
        score.clear_items()
        with pytest.raises(Exception):
            score.sse(0)
        again = items[:-12:-1]
        ids = [_add_item(score, *it) for it in again]
        assert ids == list(range(11))
        score.run()
        score.wait()
        assert [score.sse(i) for i in ids] == want[2:][:-12:-1]
        assert [score.frame_sse(k) for k in range(2)] == want[:2]
    seen = set()
    for i, (k, kind, payload) in enumerate(items):  # alone in a fresh handle: the first item of every (frame, kind)
        if (k, kind) in seen:
            continue
        seen.add((k, kind))
        with gpu(0) as solo:
            frames[k].add_to(solo)
            assert _add_item(solo, 0, kind, payload) == 0
            solo.run()
            solo.wait()
            assert solo.sse(0) == want[2 + i], (i, k, kind)
            assert solo.frame_sse(0) == want[k]


@pytest.mark.gpu
def test_rewritten_motion_and_candidate_planes_are_followed(gpu):
    """A B frame's ref0 item reads reference 1's kept warp, which the base pair makes again at every run: rewriting the base motion
    buffer between two runs is followed; so are candidate planes rewritten in place."""
    import torch

    f = _two_frames()[0]
    assert f.ft == 2
    planes = _candidate_planes(f, 0)
    with gpu(0) as score:
        f.add_to(score)
        item = _add(score, 0, "ref0", planes)
        results = []
        for step in range(3):
            if step == 1:
                f.motion.copy_(f.outputs(1, 5))
            if step == 2:
                for t, u in zip(planes[0], _candidate_planes(f, 9)[0]):
                    t.copy_(u)
            torch.cuda.synchronize()
            score.run()
            score.wait()
            want = _yardstick([(f, f.residue, f.motion), (_with_refs(f, "ref0", planes), f.residue, f.motion)])
            assert [score.frame_sse(0), score.sse(item)] == want, step
            results.append(want[1])
        assert results[0] != results[1] != results[2]


@pytest.mark.gpu
def test_refusals_on_a_handle_with_frames_and_a_run_in_flight(gpu):
    """Each refusal of ccd_iscore_add_refs on a handle that holds a P and a B frame leaves the item count as it was; between run()
    and wait() add_refs is refused with CCD_ERR_ARG and works again after the wait."""
    from cool_chic_amd import CcdError

    b, p = _two_frames()
    planes = _candidate_planes(b, 0)
    p_planes = _candidate_planes(p, 0)
    ptrs = [[t.data_ptr() for t in planes[r]] for r in range(2)]
    with gpu(0) as score:
        b.add_to(score)
        p.add_to(score)
        hole = [ptrs[0][0], 0, ptrs[0][2]]
        refused = [lambda: score.add_refs(2, ptrs[0]), lambda: score.add_refs(-1, ptrs[0]), lambda: score.add_refs(0, None, None),
                   lambda: score.add_refs(0, hole), lambda: score.add_refs(0, ptrs[0], hole),
                   lambda: score.add_refs(1, [t.data_ptr() for t in p_planes[0]], [t.data_ptr() for t in p_planes[1]]),
                   lambda: score.add_refs(1, None, [t.data_ptr() for t in p_planes[1]])]
        for i, call in enumerate(refused):
            with pytest.raises(CcdError) as e:
                call()
            assert e.value.code == ERR_ARG, i
        assert _add(score, 0, "ref1", planes) == 0
        score.run()
        with pytest.raises(CcdError) as e:
            _add(score, 0, "ref0", planes)
        assert e.value.code == ERR_ARG
        score.wait()
        assert score.sse(0) == _yardstick([(_with_refs(b, "ref1", planes), b.residue, b.motion)])[0]
        assert _add(score, 0, "ref0", planes) == 1 and _add(score, 1, "ref0", p_planes) == 2
