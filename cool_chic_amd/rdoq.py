"""RdoqStep: one requantisation step on one MI355X - from the distortion and rate delta maps of every latent, choose +-1 moves
that provably do not interact and apply them to the device latents in place (wraps the ccd_rdoq_* C ABI).

After a step the frame's squared error has changed by exactly `d_sse` and the model bits by `d_bits` (within the rate deltas'
own bound): the sums of the chosen entries of the two maps.

A step may run several rounds (`rounds`): a candidate that lost a cell of its box to a candidate that itself lost elsewhere
competes again once the winners' neighbourhoods are out of the way.  The selected set stays pairwise independent and grows
towards the set a walk over the candidates in key order would take; `StepResult.n_open == 0` says it has got there."""
import ctypes as C
from typing import List, NamedTuple, Optional, Sequence, Tuple

from ._handle import _DevArray, _Handle, ptr_array
from ._lib import CCHeader, RdoqFollow, RdoqResult, check, lib


class StepResult(NamedTuple):
    n_candidates: int
    n_moves: int
    n_moves_grid: Tuple[int, ...]
    d_sse: int      # exact: the sum of the chosen dD
    d_bits: float   # the sum of the chosen dBits
    d_cost: float   # kD * d_sse + kR * d_bits
    n_open: int = 0  # candidates of the last round that were not selected; 0: the selected set is maximal


UNCHANGED = object()  # SlotMaps.dep_ptrs: the slot's dependent maps stay what they are


class SlotMaps(NamedTuple):
    """What run_step gives one slot for one step."""
    kD: float
    kR: float
    mask: int                                   # the grids that may move (grid_mask)
    dd_ptrs: Optional[Sequence[Optional[int]]]  # per grid the distortion map; None: none, the slot's moves cost their bits
    dbits_ptrs: Sequence[int]                   # per grid the rate map
    dep_ptrs: Optional[Sequence[Optional[int]]] = UNCHANGED  # per grid the dependent map, or None: the slot has none


def grid_mask(n_grids: int, grids: Optional[Sequence[int]] = None) -> int:
    """Bit g for every grid g of `grids` (None: all) that exists."""
    return sum(1 << g for g in (range(n_grids) if grids is None else grids) if 0 <= g < n_grids)


def check_lambda(lmbda: float, min_gain: Optional[float] = None) -> None:
    """A descent's lmbda and min_gain, or a search's lmbda alone (min_gain None): finite and not negative."""
    if not all(0.0 <= float(v) < float("inf") for v in (lmbda, min_gain or 0.0)):  # (nan fails every comparison)
        raise ValueError(f"{'lmbda' if min_gain is None else 'lmbda and min_gain'} must be finite and not negative")


def run_step(rdoq, stream: int, slots: Sequence[SlotMaps], min_gain: float, rounds: int = 1) -> List[StepResult]:
    """One step of an RdoqStep whose slots are `slots`, in order: the maps of every slot, step, wait; the result of every slot."""
    for s, m in enumerate(slots):
        rdoq.set_maps(s, [None] * len(m.dbits_ptrs) if m.dd_ptrs is None else m.dd_ptrs, m.dbits_ptrs)
        if m.dep_ptrs is not UNCHANGED:
            rdoq.set_dep_maps(s, m.dep_ptrs)
    rdoq.step([m.kD for m in slots], [m.kR for m in slots], [float(min_gain)] * len(slots), [m.mask for m in slots], stream, rounds=rounds)
    rdoq.wait(stream)
    return [rdoq.result(s) for s in range(len(slots))]


def cell() -> int:
    """Luma samples per side of a cell of the claim raster (ccd_rdoq_cell)."""
    return int(lib().ccd_rdoq_cell())


def max_rounds() -> int:
    """The most rounds a step may run (ccd_rdoq_max_rounds)."""
    return int(lib().ccd_rdoq_max_rounds())


def max_follows() -> int:
    """The most follows one slot takes (ccd_rdoq_max_follows)."""
    return int(lib().ccd_rdoq_max_follows())


def lane_cells() -> int:
    """Cells of a box up to which one lane walks it in a step's kernels (ccd_rdoq_lane_cells): a cost figure."""
    return int(lib().ccd_rdoq_lane_cells())


def influence_box(arch: CCHeader, frame_data_type: int, grid: int, y: int, x: int) -> Tuple[int, int, int, int]:
    """(top, left, bottom, right), inclusive, in cells: the influence box of the latent (y, x) of `grid`
    (include/ccd.h: ccd_rdoq_influence_box).  Latents whose boxes share no cell can be moved independently.  Host only."""
    box = (C.c_int32 * 4)()
    check(lib().ccd_rdoq_influence_box(C.byref(arch), int(frame_data_type), int(grid), int(y), int(x), box), "ccd_rdoq_influence_box")
    return tuple(int(v) for v in box)


class RdoqStep(_Handle):
    """One slot per candidate: add() its device latents, set_maps() the device maps, step() + wait(), then result() and moves()."""

    influence_box = staticmethod(influence_box)

    _destroy = "ccd_rdoq_destroy"

    def __init__(self, device: int = 0):
        self._open("ccd_rdoq_create", device)

    def __len__(self):
        return len(self._grid_shapes)

    def _open(self, create, device, *args):
        super()._open(create, device, *args)
        self._cells: list = []  # per slot: the (cells_h, cells_w) of its claim raster

    def add(self, arch: CCHeader, frame_data_type: int, latent_ptrs: Sequence[int], owner=None) -> int:
        """Device latents (int8 [h][w] per grid), read AND WRITTEN by every step.  Returns the slot."""
        slot = check(lib().ccd_rdoq_add(self._h, C.byref(arch), int(frame_data_type), ptr_array(latent_ptrs)), "ccd_rdoq_add")
        self._note_grids(arch, len(latent_ptrs))
        self._cells.append((-(-int(arch.img_size[0]) // cell()), -(-int(arch.img_size[1]) // cell())))
        self._keep(owner)  # (the device latents the slot uses at step())
        return slot

    def set_maps(self, slot: int, dd_ptrs: Sequence[Optional[int]], dbits_ptrs: Sequence[int], owner=None):
        """Per grid the device int64 [2][h][w] distortion map (None / 0: zeros) and the device float32 [2][h][w] rate map."""
        n = len(self._grid_shapes[int(slot)])
        if len(dd_ptrs) != n or len(dbits_ptrs) != n:
            raise ValueError(f"slot {slot} has {n} grids")
        check(lib().ccd_rdoq_set_maps(self._h, int(slot), ptr_array(dd_ptrs), ptr_array(dbits_ptrs)), "ccd_rdoq_set_maps")
        self._keep(owner)

    def link(self, slot: int, leader: int):
        """`slot` joins the claim raster of `leader`: from the next step on the candidates of both compete as one population, so
        the moves a step selects are pairwise independent across both slots (include/ccd.h: ccd_rdoq_link).  For two cool-chics
        that decode into one frame of the same size and sample format.  On a tie of the costs the leader's candidate wins.  Results,
        move maps and masks stay per slot; a slot whose mask is 0 leaves its partner stepping as if unlinked.  There is no unlink."""
        check(lib().ccd_rdoq_link(self._h, int(slot), int(leader)), "ccd_rdoq_link")

    def follow(self, slot: int, frame_type: int, which: int, motion_ptr: int, target: int, frozen: int = -1,
               global_flow: Sequence[int] = (0, 0, 0, 0), warp_filter_size: int = 8, owner=None) -> int:
        """The frame `slot` decodes is reference `which` of a P (1) / B (2) frame F whose device motion output (float32
        [2 | 4][h][w]) is at `motion_ptr`: from the next step on a candidate of `slot` also claims, in the raster of `target` (F's
        residue slot or the leader of F's pair; mask 0 if F is held fixed), the cells whose samples can read what it changes,
        along the flows as they are at that step (include/ccd.h: ccd_rdoq_follow).  `frozen`: the slot of F's
        motion cool-chic, which a step then refuses to move.  Returns the follow's index.  There is no unfollow."""
        d = RdoqFollow(int(frame_type), int(which), int(motion_ptr) or None, (C.c_int32 * 4)(*[int(v) for v in global_flow]),
                       int(warp_filter_size), int(target), int(frozen))
        k = check(lib().ccd_rdoq_follow(self._h, int(slot), C.byref(d)), "ccd_rdoq_follow")
        self._keep(owner)
        return k

    def set_dep_maps(self, slot: int, dep_ptrs: Optional[Sequence[Optional[int]]], owner=None):
        """Per grid the device int64 [2][h][w] dependent map (DistortionDeltas.dep_delta_map), None / 0: none.  The cost of a move
        becomes (dD + dDdep) * kD + dBits * kR, and a move exists in neither map's sentinel.  None: no dependent maps."""
        if dep_ptrs is not None and len(dep_ptrs) != len(self._grid_shapes[int(slot)]):
            raise ValueError(f"slot {slot} has {len(self._grid_shapes[int(slot)])} grids")
        check(lib().ccd_rdoq_set_dep_maps(self._h, int(slot), None if dep_ptrs is None else ptr_array(dep_ptrs)), "ccd_rdoq_set_dep_maps")
        self._keep(owner)

    def dep_sse(self, slot: int) -> int:
        """After step() + wait(): the exact sum of the chosen entries of the slot's dependent maps - what the step did to the
        squared error of the frames that predict from the slot's frame.  StepResult.d_sse stays the slot's own frame's."""
        v = C.c_int64()
        check(lib().ccd_rdoq_slot_dep_sse(self._h, int(slot), C.byref(v)), "ccd_rdoq_slot_dep_sse")
        return int(v.value)

    def reach(self, slot: int, follow: int) -> _DevArray:
        """After step() + wait(): the follow's reach table of that step, uint32 [cells_h][cells_w][4] on the device:
        {top, left, ~bottom, ~right} in cells of the dependent, all ones where no sample of it reads the cell."""
        ptr = C.c_void_p()
        n = check(lib().ccd_rdoq_slot_reach(self._h, int(slot), int(follow), C.byref(ptr)), "ccd_rdoq_slot_reach")
        ch, cw = self._cells[int(slot)]
        assert ch * cw == n
        return _DevArray(ptr.value or 0, (ch, cw, 4), "<u4", self)

    def flow_boxes(self, slot: int, follow: int, grid: int) -> _DevArray:
        """After step() + wait(): uint16 [h][w][4] on the device, {top, left, bottom, right} of every latent's flow box for the
        follow; top > bottom: empty."""
        ptr = C.c_void_p()
        n = check(lib().ccd_rdoq_slot_flow_boxes(self._h, int(slot), int(follow), int(grid), C.byref(ptr)), "ccd_rdoq_slot_flow_boxes")
        h, w = self._grid_shapes[int(slot)][int(grid)]
        assert h * w == n
        return _DevArray(ptr.value or 0, (h, w, 4), "<u2", self)

    def step(self, kD: Sequence[float], kR: Sequence[float], min_gain: Sequence[float], grid_mask: Sequence[int], stream: int = 0,
             rounds: int = 1):
        """Per-slot factors of the cost dD * kD + dBits * kR, the least gain of a candidate and the grids that may move (bit g).
        `rounds` (1 .. max_rounds()): after each round the winners' boxes are taken, the candidates that meet them are dropped and
        the rest compete again (include/ccd.h: ccd_rdoq_step_rounds); 1 is the single selection.  Only enqueues."""
        n = len(self)
        if not (len(kD) == len(kR) == len(min_gain) == len(grid_mask) == n):
            raise ValueError(f"the handle holds {n} slots")
        check(lib().ccd_rdoq_step_rounds(self._h, (C.c_double * n)(*[float(v) for v in kD]), (C.c_double * n)(*[float(v) for v in kR]),
                                         (C.c_double * n)(*[float(v) for v in min_gain]), (C.c_uint64 * n)(*[int(v) for v in grid_mask]),
                                         int(rounds), C.c_void_p(stream or None)), "ccd_rdoq_step_rounds")

    def wait(self, stream: int = 0):
        check(lib().ccd_rdoq_wait(self._h, C.c_void_p(stream or None)), "ccd_rdoq_wait")

    def result(self, slot: int) -> StepResult:
        r = RdoqResult()
        check(lib().ccd_rdoq_slot_result(self._h, int(slot), C.byref(r)), "ccd_rdoq_slot_result")
        n_open = check(lib().ccd_rdoq_slot_open(self._h, int(slot)), "ccd_rdoq_slot_open")
        return StepResult(int(r.n_candidates), int(r.n_moves), tuple(int(r.n_moves_grid[g]) for g in range(r.n_grids)), int(r.d_sse),
                          float(r.d_bits), float(r.d_cost), int(n_open))

    def moves(self, slot: int, grid: int) -> _DevArray:
        """After step() + wait(): int8 [h][w] on the device, the move (-1, 0, +1) the step applied at every latent of the grid.
        Valid until the next step / close."""
        return self._grid_map("ccd_rdoq_slot_moves", slot, grid, "|i1")
