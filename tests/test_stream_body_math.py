"""The coding order of a latent grid and the arithmetic the pipelined entropy kernel's streamed body rests on, checked on the
CPU against the code the kernels and both writers compile (cool_chic_amd/csrc/ccd_wavefront.hpp, through the host-only export
ccd_debug_grid_walk) and against the wavefront order itself as this file enumerates it (latent.py:66-140: pixels of a step share
x + 10 y, steps in increasing order, rows top to bottom inside a step; raster order up to 9 columns):

* StepWalk (incremental, with its multiply-shift for x / 10), StepIter and the free functions walk every grid in that order,
  step by step, and StepWalk's closed forms (seek_before with len_of / moved_at: the state a producer starts a segment from)
  give the same y0, x0, n, moved and left at every step;
* grid_segments cuts a grid into ramp / body / ramp exactly where StreamBody::init's rule says, and the segments partition the
  steps and the pixels;
* the steps [230, W + 10 (H - 24)) of a grid with W > 230 and H >= 25 all hold >= 23 pixels, the 230 steps in front of them
  and the 230 behind them hold 2 760 pixels each (closed forms of StreamBody::init);
* in that body a pixel's left neighbour lies >= 18 places earlier in decoding order, i.e. in an EARLIER 16-pixel batch than any
  8-pixel task that holds the pixel - the condition under which batches may be cut without regard to step ends;
* the left neighbour of the pixel with index i of a step is the pixel with index i (+ 1 when the step start moved down a row)
  of the previous step, and an 8-pixel task of the stream holds pixels of at most two steps - what the producers' task header
  computes per lane."""
import ctypes as C

import numpy as np
import pytest

from cool_chic_amd._lib import lib

CCD_ERR_ARG = -7  # include/ccd.h
RAMP_TASK_PIX = 4  # CCD_RAMP_TASK_PIX


@pytest.fixture(scope="module")
def T():
    """kStreamMinStep of the library under test."""
    return int(lib().ccd_debug_stream_min_step())


def wavefront(h, w):
    """(step index, y, x) of every pixel in decoding order, and the first pixel's stream position per step."""
    order = []
    starts = []
    for c in range(w + 10 * (h - 1)):
        starts.append(len(order))
        y0 = 0 if c < w else (c - w) // 10 + 1
        x0 = c if c < w else w - 10 + (c - w) % 10
        n = min(h - y0, x0 // 10 + 1)
        for i in range(n):
            order.append((c, y0 + i, x0 - 10 * i))
    return order, starts


def step_table(h, w):
    """[n_steps][3] = y0, x0, n of every step: wavefront(h, w), or a plain raster for a grid at most 9 wide."""
    if w <= 9:
        return np.array([(p // w, p % w, 1) for p in range(h * w)], np.int64)
    order, starts = wavefront(h, w)
    lens = np.diff(np.array(starts + [len(order)]))
    return np.array([(order[s][1], order[s][2], n) for s, n in zip(starts, lens)], np.int64)


def grid_walk(h, w, task_pix, which, with_steps=True):
    """ccd_debug_grid_walk -> (return value, steps [n][5], segments [n_segs][6])."""
    n = lib().ccd_debug_grid_walk(h, w, task_pix, which, None, 0, None, None)
    if n < 0:
        return n, None, None
    steps = np.full((n, 5), -99, np.int32)
    segs = np.full((3, 6), -99, np.int32)
    n_segs = C.c_int32(-99)
    rc = lib().ccd_debug_grid_walk(h, w, task_pix, which, steps.ctypes.data if with_steps else None, n, segs.ctypes.data, C.byref(n_segs))
    assert rc == n
    return n, steps, segs[:n_segs.value]


BODY_SHAPES = [(25, 241), (25, 250), (33, 480), (40, 271), (64, 521), (300, 241), (57, 332), (128, 256), (96, 768)]
EDGE_SHAPES = [(1, 1), (1, 9), (3, 9), (1, 10), (2, 10), (1, 11), (2, 11), (3, 19), (2, 20), (5, 21), (12, 37), (7, 16383), (2, 16380)]


@pytest.mark.parametrize("h,w", EDGE_SHAPES + BODY_SHAPES)
def test_coding_order_of_every_walk(h, w):
    want = step_table(h, w)
    n_steps = len(want)
    assert want[:, 2].min() >= 1 and want[:, 2].sum() == h * w
    c = np.arange(n_steps)
    pitch = w if w <= 9 else 10  # a raster grid moves down a row every w steps
    moved = ((c >= w) & ((c - w) % pitch == 0)).astype(np.int64)
    left = n_steps - 1 - c
    got = {}
    for which in range(5):  # (4: every row is what seek_before / len_of / moved_at compute, none of it next()'s)
        n, steps, _ = grid_walk(h, w, 8, which)
        assert n == n_steps, which
        got[which] = steps
        assert (steps[:, :3] == want).all(), which               # y0, x0, n: the order itself
        assert (steps[:, 2] >= 1).all() and steps[:, 2].sum() == h * w, which
        if which != 1:                                           # StepIter keeps neither
            assert (steps[:, 3] == moved).all(), which
            assert (steps[:, 4] == left).all() and steps[-1, 4] == 0, which
        else:
            assert (steps[:, 3:] == 0).all()
    for which in (1, 2, 3, 4):
        assert (got[which][:, :3] == got[0][:, :3]).all()
    for which in (2, 3, 4):
        assert (got[which] == got[0]).all()


def body_rule(h, w, task_pix, T):
    """Whether the grid has a streamed body, and why, as StreamBody::init states the rule."""
    n_pl = (w - 1) // 10 + 1
    tail = n_pl & 7
    if task_pix != 8:
        return False, "task_pix"
    if h < T:
        return False, "H < T"
    if not w > 10 * (T - 1):
        return False, "W <= 10 (T - 1)"
    if n_pl >= 48:
        return True, "n_pl >= 48"
    if 1 <= tail <= 4:
        return True, "tail %d" % tail
    return False, "tail %d" % tail


@pytest.mark.parametrize("task_pix", [2, 4, 8])
# (why24: what StreamBody::init's rule gives for 8-pixel tasks at kStreamMinStep = 24, derived by body_rule below.  H = 24 is the
# smallest height WITH a body - the rule is H >= T - so 23 is the row of the "H < T" edge and 24 its other side.)
@pytest.mark.parametrize("h,w,why24", [(23, 241, "H < T"), (24, 241, "tail 1"), (25, 230, "W <= 10 (T - 1)"), (25, 241, "tail 1"), (25, 250, "tail 1"),
                                       (40, 271, "tail 4"), (33, 480, "n_pl >= 48"), (40, 281, "tail 5")])
def test_grid_segments(h, w, why24, task_pix, T):
    on, why = body_rule(h, w, task_pix, T)
    if T == 24 and task_pix == 8:
        assert why == why24  # the shape sits on the edge it was chosen for
    order, starts = wavefront(h, w)
    n_steps = len(starts)
    lens = np.diff(np.array(starts + [len(order)]))
    n, _, segs = grid_walk(h, w, task_pix, 0, with_steps=False)
    assert n == n_steps
    assert len(segs) == (3 if on else 1)
    # the segments partition the steps and the pixels
    assert segs[0][0] == 0 and segs[-1][0] + segs[-1][1] == n_steps
    for a, b in zip(segs[:-1], segs[1:]):
        assert a[0] + a[1] == b[0]
    for first, steps, pix_before, n_pix, seg_task_pix, body in segs:
        assert steps >= 1
        assert pix_before == starts[first]
        assert n_pix == lens[first:first + steps].sum()
    assert sum(s[3] for s in segs) == h * w
    # only 8-pixel tasks are streamed; the ramps around a body run CCD_RAMP_TASK_PIX, everything else the grid's tasks
    assert [int(s[5]) for s in segs] == ([0, 1, 0] if on else [0])
    assert [int(s[4]) for s in segs] == ([RAMP_TASK_PIX, task_pix, RAMP_TASK_PIX] if on else [task_pix])
    if on:
        assert task_pix == 8
        first, steps = int(segs[1][0]), int(segs[1][1])
        assert first == 10 * (T - 1) and first + steps == w + 10 * (h - T)
        assert lens[first:first + steps].min() >= T - 1 and lens[:first].max() < T


def test_grid_walk_arguments():
    L = lib()
    assert L.ccd_debug_grid_walk(0, 20, 8, 0, None, 0, None, None) == CCD_ERR_ARG
    assert L.ccd_debug_grid_walk(20, 16384, 8, 0, None, 0, None, None) == CCD_ERR_ARG
    assert L.ccd_debug_grid_walk(20, 20, 3, 0, None, 0, None, None) == CCD_ERR_ARG
    for which in range(5):
        assert L.ccd_debug_grid_walk(3, 19, 8, which, None, 0, None, None) == 19 + 10 * 2   # steps == NULL: the count
        assert L.ccd_debug_grid_walk(3, 9, 8, which, None, 0, None, None) == 27
    # a short buffer is filled up to `cap` and no further
    steps = np.full((4, 5), -99, np.int32)
    assert L.ccd_debug_grid_walk(3, 19, 8, 0, steps.ctypes.data, 3, None, None) == 39
    assert (steps[:3, 2] == 1).all() and (steps[3] == -99).all()


@pytest.mark.parametrize("h,w", BODY_SHAPES)
def test_streamed_body_closed_forms_and_dependency_distance(h, w, T):
    order, starts = wavefront(h, w)
    n_steps = w + 10 * (h - 1)
    first, end = 10 * (T - 1), w + 10 * (h - T)
    assert first < end <= n_steps
    lens = np.diff(np.array(starts + [len(order)]))
    assert lens[first:end].min() >= T - 1
    assert starts[first] == 5 * T * (T - 1)
    assert T != 24 or starts[first] == 2760
    assert len(order) - starts[end] == starts[first] if end < n_steps else True
    assert starts[end] - starts[first] == h * w - 2 * starts[first]
    pos = {(y, x): p for p, (_, y, x) in enumerate(order)}
    body0 = starts[first]
    for p in range(starts[first], starts[end]):
        c, y, x = order[p]
        if x == 0:
            continue
        left = pos[(y, x - 1)]
        assert order[left][0] == c - 1                      # the left neighbour is decoded one step earlier ...
        i = p - starts[c]
        moved = 1 if (c >= w and (c - w) % 10 == 0) else 0
        assert left - starts[c - 1] == i + moved            # ... at the same index (+ 1 when the step start moved down a row)
        assert p - left >= 18
        task_first = body0 + ((p - body0) // 8) * 8         # first pixel of the stream task that holds p
        batch_first = body0 + ((p - body0) // 16) * 16
        assert left < batch_first and left < task_first     # an earlier batch: decoded before this task's batch can start
        # a task holds pixels of at most two steps
        last = min(task_first + 7, starts[end] - 1)
        assert order[last][0] - order[task_first][0] <= 1
