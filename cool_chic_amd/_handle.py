"""What the wrappers of the library's device handles share (DecodeBatch, EncodeBatch, QualityMeter, PngPacker, DistortionDeltas,
RdoqStep): the life of the handle, pointer marshalling and views of library-owned device memory."""
import ctypes as C
from typing import List, Sequence, Tuple

from ._lib import CCHeader, check, lib


class _DevArray:
    """Zero-copy view of library-owned device memory for torch.as_tensor(..., device='cuda')."""

    def __init__(self, ptr: int, shape: Tuple[int, ...], typestr: str, owner):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2, "strides": None}
        self._owner = owner  # keeps the batch (and its arena) alive


def dev_ptr(array) -> int:
    """The device address of a _DevArray, or of anything else with a __cuda_array_interface__."""
    return int(array.__cuda_array_interface__["data"][0])


def ptr_array(ptrs: Sequence) -> C.Array:
    """A c_void_p array of the addresses in `ptrs`, in order; None / 0 becomes NULL."""
    return (C.c_void_p * len(ptrs))(*[int(p) if p else None for p in ptrs])


class _Handle:
    """A handle of the C ABI on one device.  A subclass names the library's destroy function in `_destroy` and opens the handle
    with _open() in its __init__; close() is idempotent, also runs when the object is collected or a `with` block is left, and
    lets go of whatever was kept alive for the handle."""

    _destroy = ""            # e.g. "ccd_batch_destroy"
    _library = staticmethod(lib)  # where the create / destroy functions are looked up

    def _open(self, create: str, device: int, *args) -> None:
        """create(device, *args, &handle) of the library."""
        self._h = C.c_void_p()
        self._owners: List[object] = []  # whatever owns device memory the handle reads or writes when it runs
        self._grid_shapes: List[List[Tuple[int, int]]] = []  # per slot, per grid (h, w): the shape of a map of the grid
        check(getattr(self._library(), create)(int(device), *args, C.byref(self._h)), create)
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            getattr(self._library(), self._destroy)(self._h)
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

    def _keep(self, owner) -> None:
        if owner is not None:
            self._owners.append(owner)

    def _note_grids(self, arch: CCHeader, n_grids: int) -> None:
        """A slot was added whose grids `arch` describes."""
        self._grid_shapes.append([(int(arch.grid_h[g]), int(arch.grid_w[g])) for g in range(n_grids)])

    def _grid_map(self, getter: str, slot: int, grid: int, typestr: str, planes: Tuple[int, ...] = ()) -> _DevArray:
        """The device map [*planes][h][w] of (slot, grid) that the library's `getter` hands out."""
        ptr = C.c_void_p()
        n = check(getattr(self._library(), getter)(self._h, int(slot), int(grid), C.byref(ptr)), getter)
        h, w = self._grid_shapes[int(slot)][int(grid)]
        assert h * w == n, "the architecture given to add() does not describe the grids the library derived"
        return _DevArray(ptr.value or 0, tuple(planes) + (h, w), typestr, self)
