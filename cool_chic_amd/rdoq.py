"""RdoqStep: one requantisation step on one MI355X - from the distortion and rate delta maps of every latent, choose +-1 moves
that provably do not interact and apply them to the device latents in place (wraps the ccd_rdoq_* C ABI).

After a step the frame's squared error has changed by exactly `d_sse` and the model bits by `d_bits` (within the rate deltas'
own bound): the sums of the chosen entries of the two maps."""
import ctypes as C
from typing import List, NamedTuple, Optional, Sequence, Tuple

from ._lib import CCHeader, RdoqResult, check, lib
from .batch import _DevArray


class StepResult(NamedTuple):
    n_candidates: int
    n_moves: int
    n_moves_grid: Tuple[int, ...]
    d_sse: int      # exact: the sum of the chosen dD
    d_bits: float   # the sum of the chosen dBits
    d_cost: float   # kD * d_sse + kR * d_bits


def cell() -> int:
    """Luma samples per side of a cell of the claim raster (ccd_rdoq_cell)."""
    return int(lib().ccd_rdoq_cell())


def influence_box(arch: CCHeader, frame_data_type: int, grid: int, y: int, x: int) -> Tuple[int, int, int, int]:
    """(top, left, bottom, right), inclusive, in cells: the influence box of the latent (y, x) of `grid`
    (include/ccd.h: ccd_rdoq_influence_box).  Latents whose boxes share no cell can be moved independently.  Host only."""
    box = (C.c_int32 * 4)()
    check(lib().ccd_rdoq_influence_box(C.byref(arch), int(frame_data_type), int(grid), int(y), int(x), box), "ccd_rdoq_influence_box")
    return tuple(int(v) for v in box)


class RdoqStep:
    """One slot per candidate: add() its device latents, set_maps() the device maps, step() + wait(), then result() and moves()."""

    influence_box = staticmethod(influence_box)

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        check(lib().ccd_rdoq_create(int(device), C.byref(self._h)), "ccd_rdoq_create")
        self.device = int(device)
        self._owners: List[object] = []  # whatever owns the device latents and maps the slots use at step()
        self._grid_shapes: List[List[Tuple[int, int]]] = []

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().ccd_rdoq_destroy(self._h)
            self._h = C.c_void_p()
            self._owners = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __len__(self):
        return len(self._grid_shapes)

    def add(self, arch: CCHeader, frame_data_type: int, latent_ptrs: Sequence[int], owner=None) -> int:
        """Device latents (int8 [h][w] per grid), read AND WRITTEN by every step.  Returns the slot."""
        lat = (C.c_void_p * len(latent_ptrs))(*[int(p) for p in latent_ptrs])
        slot = check(lib().ccd_rdoq_add(self._h, C.byref(arch), int(frame_data_type), lat), "ccd_rdoq_add")
        self._grid_shapes.append([(int(arch.grid_h[g]), int(arch.grid_w[g])) for g in range(len(latent_ptrs))])
        if owner is not None:
            self._owners.append(owner)
        return slot

    def set_maps(self, slot: int, dd_ptrs: Sequence[Optional[int]], dbits_ptrs: Sequence[int], owner=None):
        """Per grid the device int64 [2][h][w] distortion map (None / 0: zeros) and the device float32 [2][h][w] rate map."""
        n = len(self._grid_shapes[int(slot)])
        if len(dd_ptrs) != n or len(dbits_ptrs) != n:
            raise ValueError(f"slot {slot} has {n} grids")
        dd = (C.c_void_p * n)(*[int(p) if p else None for p in dd_ptrs])
        db = (C.c_void_p * n)(*[int(p) if p else None for p in dbits_ptrs])
        check(lib().ccd_rdoq_set_maps(self._h, int(slot), dd, db), "ccd_rdoq_set_maps")
        if owner is not None:
            self._owners.append(owner)

    def step(self, kD: Sequence[float], kR: Sequence[float], min_gain: Sequence[float], grid_mask: Sequence[int], stream: int = 0):
        """Per-slot factors of the cost dD * kD + dBits * kR, the least gain of a candidate and the grids that may move (bit g).
        Only enqueues."""
        n = len(self)
        if not (len(kD) == len(kR) == len(min_gain) == len(grid_mask) == n):
            raise ValueError(f"the handle holds {n} slots")
        check(lib().ccd_rdoq_step(self._h, (C.c_double * n)(*[float(v) for v in kD]), (C.c_double * n)(*[float(v) for v in kR]),
                                  (C.c_double * n)(*[float(v) for v in min_gain]), (C.c_uint64 * n)(*[int(v) for v in grid_mask]),
                                  C.c_void_p(stream or None)), "ccd_rdoq_step")

    def wait(self, stream: int = 0):
        check(lib().ccd_rdoq_wait(self._h, C.c_void_p(stream or None)), "ccd_rdoq_wait")

    def result(self, slot: int) -> StepResult:
        r = RdoqResult()
        check(lib().ccd_rdoq_slot_result(self._h, int(slot), C.byref(r)), "ccd_rdoq_slot_result")
        return StepResult(int(r.n_candidates), int(r.n_moves), tuple(int(r.n_moves_grid[g]) for g in range(r.n_grids)), int(r.d_sse),
                          float(r.d_bits), float(r.d_cost))

    def moves(self, slot: int, grid: int) -> _DevArray:
        """After step() + wait(): int8 [h][w] on the device, the move (-1, 0, +1) the step applied at every latent of the grid.
        Valid until the next step / close."""
        ptr = C.c_void_p()
        n = check(lib().ccd_rdoq_slot_moves(self._h, int(slot), int(grid), C.byref(ptr)), "ccd_rdoq_slot_moves")
        h, w = self._grid_shapes[int(slot)][int(grid)]
        assert h * w == n, "the architecture given to add() does not describe the grids the library derived"
        return _DevArray(ptr.value or 0, (h, w), "|i1", self)
