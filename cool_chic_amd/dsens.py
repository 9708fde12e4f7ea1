"""DistortionDeltas: what moving ONE latent by -1 / +1 does to the squared error of the decoded planes, for every latent of
every grid, on one MI355X (wraps the ccd_dsens_* C ABI).

The numbers are those of one decode per moved latent (DecodeBatch.add_latents + QualityMeter), as integers; they come from a
few thousand passes of the float path per picture, each of which moves every latent of one lattice at once."""
import ctypes as C
from typing import Optional, Sequence

from ._handle import _DevArray, _Handle, ptr_array
from ._lib import CCHeader, DsensDependent, DsensInter, check, lib

SENTINEL = -2 ** 63  # the entry where v - 1 / v + 1 leaves [-64, 63] (INT64_MIN)


def latent_footprint(arch: CCHeader, grid: int):
    """(top, left, bottom, right) in luma samples around the latent (0, 0) of `grid` (include/ccd.h: ccd_latent_footprint),
    or None for a hyperlatent grid.  Host only."""
    box = (C.c_int32 * 4)()
    rc = check(lib().ccd_latent_footprint(C.byref(arch), int(grid), box), "ccd_latent_footprint")
    return None if rc == 1 else tuple(int(v) for v in box)


def probe_stride(arch: CCHeader, grid: int, frame_data_type: int = 0, margin: int = 0) -> int:
    """The lattice stride of the grid's passes (ccd_latent_probe_stride_margin); 0 for a hyperlatent grid.  `margin`: samples kept
    between the regions of two latents a stride apart - 0 for a slot without dependents, dependent_margin() for one with.  Host only."""
    return check(lib().ccd_latent_probe_stride_margin(C.byref(arch), int(grid), int(frame_data_type), int(margin)),
                 "ccd_latent_probe_stride_margin")


def dependent_margin(frame_data_type: int, warp_filter_sizes: Sequence[int]) -> int:
    """The margin a slot with dependents plans its passes with: W - 1 for rgb / yuv444, W + 2 for yuv420, W the
    widest window of the dependents' warps (2 bilinear, 4 bicubic, the filter size for sinc)."""
    w = max(int(t) for t in warp_filter_sizes)
    return w + 2 if int(frame_data_type) == 1 else w - 1


class DistortionDeltas(_Handle):
    """One slot per candidate; run() enqueues every pass of every slot, wait() ends it, delta_map() hands out the maps."""

    _destroy = "ccd_dsens_destroy"

    def __init__(self, device: int = 0, n_probe_slots: int = 16):
        self._open("ccd_dsens_create", device, int(n_probe_slots))

    def __len__(self):
        return len(self._grid_shapes)

    def add(self, arch: CCHeader, bytes_nn: bytes, latent_ptrs: Sequence[int], source_ptrs: Sequence[int], bitdepth: int,
            frame_data_type: int, owner=None) -> int:
        """Device latents (int8 [h][w] per grid, read at every run, never written) and the three device planes of the source
        (uint8 at 8 bits, else uint16; half-size chroma for yuv420).  Returns the slot."""
        src = (C.c_void_p * 3)(*[int(p) for p in source_ptrs])
        slot = check(lib().ccd_dsens_add(self._h, C.byref(arch), bytes_nn, len(bytes_nn), ptr_array(latent_ptrs), src, int(bitdepth),
                                         int(frame_data_type)), "ccd_dsens_add")
        self._note_grids(arch, len(latent_ptrs))
        self._keep(owner)  # (the device latents and source planes the slot reads at run())
        return slot

    def add_inter(self, arch: CCHeader, bytes_nn: bytes, latent_ptrs: Sequence[int], source_ptrs: Sequence[int], bitdepth: int,
                  frame_data_type: int, frame_type: int, role: int, partner_ptr: int, ref0_ptrs: Sequence[int],
                  ref1_ptrs: Optional[Sequence[int]] = None, global_flow: Sequence[int] = (0, 0, 0, 0), warp_filter_size: int = 8,
                  owner=None) -> int:
        """One cool-chic of a P / B frame (ccd_dsens_add_inter): `role` 0 the frame's residue cool-chic,
        1 its motion cool-chic; `partner_ptr` the device f32 synthesis output of the OTHER one (read at every run, held fixed);
        ref0_ptrs / ref1_ptrs the device planes of the references (ref1: B frames, frame_type 2); source planes, bitdepth and
        frame_data_type are the FRAME's.  The maps are those of one ccd_inter_reconstruct per moved latent.  Returns the slot."""
        src = (C.c_void_p * 3)(*[int(p) for p in source_ptrs])
        gf = [int(v) for v in global_flow] + [0] * 4
        it = DsensInter(frame_type=int(frame_type), role=int(role), partner=int(partner_ptr) or None,
                        ref0=(C.c_void_p * 3)(*[int(p) or None for p in ref0_ptrs]),
                        ref1=(C.c_void_p * 3)(*[int(p) or None for p in (ref1_ptrs or (0, 0, 0))]),
                        global_flow=(C.c_int32 * 4)(*gf[:4]), warp_filter_size=int(warp_filter_size))
        slot = check(lib().ccd_dsens_add_inter(self._h, C.byref(arch), bytes_nn, len(bytes_nn), ptr_array(latent_ptrs), src, int(bitdepth),
                                               int(frame_data_type), C.byref(it)), "ccd_dsens_add_inter")
        self._note_grids(arch, len(latent_ptrs))
        self._keep(owner)  # (latents, source, partner and reference planes: all read at run())
        return slot

    def run(self, stream: int = 0):
        check(lib().ccd_dsens_run(self._h, C.c_void_p(stream or None)), "ccd_dsens_run")

    def wait(self, stream: int = 0):
        check(lib().ccd_dsens_wait(self._h, C.c_void_p(stream or None)), "ccd_dsens_wait")

    def passes(self, slot: int) -> int:
        """Passes of the float path one run spends on the slot."""
        return check(lib().ccd_dsens_passes(self._h, int(slot)), "ccd_dsens_passes")

    def delta_map(self, slot: int, grid: int) -> _DevArray:
        """After run() + wait(): int64 [2][h][w], the change of the frame's squared error if the latent at (y, x) alone were
        v - 1 (plane 0) or v + 1 (plane 1); SENTINEL where that leaves [-64, 63].  Valid until the next run / close."""
        return self._grid_map("ccd_dsens_slot_map", slot, grid, "<i8", (2,))

    def add_dependent(self, slot: int, frame_type: int, which: int, residue_ptr: int, motion_ptr: int, source_ptrs: Sequence[int],
                      other_ref_ptrs: Optional[Sequence[int]] = None, global_flow: Sequence[int] = (0, 0, 0, 0),
                      warp_filter_size: int = 8, owner=None) -> None:
        """A P / B frame that predicts from the frame of `slot` as its reference number `which` (ccd_dsens_add_dependent,
        DESIGN.md section 4.16): the device f32 outputs of its residue and motion cool-chics, the device planes of its source and,
        for a B frame, of its OTHER reference - all read at every run and held fixed.  Size, bit depth and frame_data_type are the
        slot's.  The slot's passes are planned again with the wider stride (passes())."""
        gf = [int(v) for v in global_flow] + [0] * 4
        dep = DsensDependent(frame_type=int(frame_type), which=int(which), residue=int(residue_ptr) or None, motion=int(motion_ptr) or None,
                             other_ref=(C.c_void_p * 3)(*[int(p) or None for p in (other_ref_ptrs or (0, 0, 0))]),
                             src=(C.c_void_p * 3)(*[int(p) or None for p in source_ptrs]),
                             global_flow=(C.c_int32 * 4)(*gf[:4]), warp_filter_size=int(warp_filter_size))
        check(lib().ccd_dsens_add_dependent(self._h, int(slot), C.byref(dep)), "ccd_dsens_add_dependent")
        self._keep(owner)

    def dep_delta_map(self, slot: int, grid: int) -> _DevArray:
        """After run() + wait(): int64 [2][h][w], the change of the summed squared error of the slot's DEPENDENTS if the latent
        at (y, x) alone were v - 1 / v + 1; SENTINEL where that leaves [-64, 63] and at conflicts (dep_conflicts)."""
        return self._grid_map("ccd_dsens_slot_dep_map", slot, grid, "<i8", (2,))

    def dep_conflicts(self, slot: int, grid: int) -> int:
        """Legal entries of dep_delta_map(slot, grid) that are SENTINEL because a unit of a dependent read the regions of two
        latents of one pass."""
        return check(lib().ccd_dsens_slot_dep_conflicts(self._h, int(slot), int(grid)), "ccd_dsens_slot_dep_conflicts")
