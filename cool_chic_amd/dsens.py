"""DistortionDeltas: what moving ONE latent by -1 / +1 does to the squared error of the decoded planes, for every latent of
every grid, on one MI355X (wraps the ccd_dsens_* C ABI).

The numbers are those of one decode per moved latent (DecodeBatch.add_latents + QualityMeter), as integers; they come from a
few thousand passes of the float path per picture, each of which moves every latent of one lattice at once."""
import ctypes as C
from typing import Optional, Sequence

from ._handle import _DevArray, _Handle, ptr_array
from ._lib import CCHeader, DsensInter, check, lib

SENTINEL = -2 ** 63  # the entry where v - 1 / v + 1 leaves [-64, 63] (INT64_MIN)


def latent_footprint(arch: CCHeader, grid: int):
    """(top, left, bottom, right) in luma samples around the latent (0, 0) of `grid` (include/ccd.h: ccd_latent_footprint),
    or None for a hyperlatent grid.  Host only."""
    box = (C.c_int32 * 4)()
    rc = check(lib().ccd_latent_footprint(C.byref(arch), int(grid), box), "ccd_latent_footprint")
    return None if rc == 1 else tuple(int(v) for v in box)


def probe_stride(arch: CCHeader, grid: int, frame_data_type: int = 0) -> int:
    """The lattice stride of the grid's passes (ccd_latent_probe_stride); 0 for a hyperlatent grid.  Host only."""
    return check(lib().ccd_latent_probe_stride(C.byref(arch), int(grid), int(frame_data_type)), "ccd_latent_probe_stride")


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
