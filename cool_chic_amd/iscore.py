"""InterScore: the squared error of many candidates of P / B frames per launch, on one MI355X (wraps the ccd_iscore_* C ABI;
DESIGN.md section 4.19).

A frame is a P / B frame as InterRdEvaluator reconstructs it - the float outputs of its two cool-chics, its references, its source;
an item is that frame with ONE of the two outputs replaced.  The numbers are those of ccd_inter_reconstruct followed by
QualityMeter.score_planes, as integers, without a plane being stored.

A reference item (add_refs; section 4.22) is the frame's own pair reconstructed against OTHER reference planes - what a candidate
of the frame it predicts from decodes to - in the same index space and with the same kind of result."""
import ctypes as C
from typing import List, Optional, Sequence, Tuple

from ._handle import _Handle
from ._lib import IScoreFrame, check, lib


def _ptrs3(ptrs: Optional[Sequence[int]]):
    return (C.c_void_p * 3)(*[int(p) or None for p in (ptrs or (0, 0, 0))])


class InterScore(_Handle):
    """add_frame() the frames, add() / add_refs() candidates, run() + wait(), then frame_sse() / sse(); clear_items() keeps the frames."""

    _destroy = "ccd_iscore_destroy"

    def __init__(self, device: int = 0):
        self._open("ccd_iscore_create", device)
        self._item_owners: List[object] = []

    def add_frame(self, frame_type: int, h: int, w: int, bitdepth: int, frame_data_type: int, residue_ptr: int, motion_ptr: int,
                  ref0_ptrs: Sequence[int], ref1_ptrs: Optional[Sequence[int]], source_ptrs: Sequence[int],
                  global_flow: Sequence[int] = (0, 0, 0, 0), warp_filter_size: int = 8, owner=None) -> int:
        """A P (1) / B (2) frame: the device f32 outputs of its residue and motion cool-chics (the base pair), the device planes
        of its references (ref1: B frames) and of its source (uint8 at 8 bits, else uint16; half-size chroma for yuv420,
        frame_data_type 1).  Everything is read at every run and never written; `owner` keeps it alive.  Returns the frame."""
        gf = [int(v) for v in global_flow] + [0] * 4
        d = IScoreFrame(frame_type=int(frame_type), h=int(h), w=int(w), bitdepth=int(bitdepth), frame_data_type=int(frame_data_type),
                        residue=int(residue_ptr) or None, motion=int(motion_ptr) or None, ref0=_ptrs3(ref0_ptrs), ref1=_ptrs3(ref1_ptrs),
                        src=_ptrs3(source_ptrs), global_flow=(C.c_int32 * 4)(*gf[:4]), warp_filter_size=int(warp_filter_size))
        frame = check(lib().ccd_iscore_add_frame(self._h, C.byref(d)), "ccd_iscore_add_frame")
        self._keep(owner)
        return frame

    def add(self, frame: int, role: int, output_ptr: int, owner=None) -> int:
        """The frame with the output of its residue (role 0) or motion (role 1) cool-chic replaced by the device f32 tensor at
        `output_ptr` ([4 | 5][h][w] / [2 | 4][h][w]).  Returns the item."""
        item = check(lib().ccd_iscore_add(self._h, int(frame), int(role), C.c_void_p(int(output_ptr) or None)), "ccd_iscore_add")
        if owner is not None:
            self._item_owners.append(owner)
        return item

    def add_refs(self, frame: int, ref0_ptrs: Optional[Sequence[int]] = None, ref1_ptrs: Optional[Sequence[int]] = None, owner=None) -> int:
        """The frame's base pair against the device integer planes `ref0_ptrs` in place of reference 0 and / or `ref1_ptrs` in
        place of reference 1 (B frames); None: the frame's own reference.  Layout of add_frame's references; read at every run,
        never written.  Returns the item, in the index space of add()."""
        r0 = None if ref0_ptrs is None else _ptrs3(ref0_ptrs)
        r1 = None if ref1_ptrs is None else _ptrs3(ref1_ptrs)
        item = check(lib().ccd_iscore_add_refs(self._h, int(frame), r0, r1), "ccd_iscore_add_refs")
        if owner is not None:
            self._item_owners.append(owner)
        return item

    def clear_items(self) -> None:
        check(lib().ccd_iscore_clear_items(self._h), "ccd_iscore_clear_items")
        self._item_owners = []

    def close(self):
        super().close()
        self._item_owners = []

    def run(self, stream: int = 0) -> None:
        check(lib().ccd_iscore_run(self._h, C.c_void_p(stream or None)), "ccd_iscore_run")

    def wait(self, stream: int = 0) -> None:
        check(lib().ccd_iscore_wait(self._h, C.c_void_p(stream or None)), "ccd_iscore_wait")

    def _result(self, getter: str, index: int) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
        sse, n = (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
        check(getattr(lib(), getter)(self._h, int(index), sse, n), getter)
        return tuple(int(v) for v in sse), tuple(int(v) for v in n)

    def frame_sse(self, frame: int) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
        """After run() + wait(): (sse per plane, samples per plane) of the frame's base pair."""
        return self._result("ccd_iscore_frame_result", frame)

    def sse(self, item: int) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
        """After run() + wait(): (sse per plane, samples per plane) of an item."""
        return self._result("ccd_iscore_result", item)
