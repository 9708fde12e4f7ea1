"""EncodeBatch: range-encodes the latents of many cool-chics on one MI355X (wraps the ccd_enc_* C ABI).

The bytes are those of writer.encode_coolchic (cool-chic header + NN payload + range-coded latents,
bitstream/encode.py:83-92); the contexts of every pixel are evaluated at once and one wave per slot runs the range
encoder's interval chain."""
import ctypes as C
from typing import NamedTuple, Sequence, Tuple

import numpy as np

from ._handle import _DevArray, _Handle, ptr_array
from ._lib import CcdError, CCHeader, EncRate, check, lib
from .batch import DecodeBatch


class SlotRate(NamedTuple):
    """What measure() found for one slot: model bits (24 - log2 of the coder's interval width, summed) per latent grid."""
    status: int             # 0, or the slot's error (the arrays are then zero)
    bits: np.ndarray        # float64 [n_grids]
    sum_width: np.ndarray   # uint64 [n_grids]: exact sum of the interval widths
    n_symbols: np.ndarray   # int64 [n_grids]
    total_bits: float       # bits summed in grid order on the device
    n_bytes_nn: int
    n_bytes_header: int


class ParamDeltas(NamedTuple):
    """What measure_param_deltas() found for one slot: rows are the ARM integers first .. first + len - 1, columns -1 and +1."""
    first: int
    bits: np.ndarray        # float64 [count][2]: change of total_bits; +inf: the move cannot be transmitted
    sum_width: np.ndarray   # int64 [count][2]: exact change of the sum of interval widths
    moved: np.ndarray       # int64 [count][2]: symbols whose width changed


class EncodeBatch(_Handle):
    """One slot per cool-chic; run() encodes all of them in the same two launches, measure() prices them without the chain."""

    _destroy = "ccd_enc_destroy"

    def __init__(self, device: int = 0):
        self._open("ccd_enc_create", device)

    def __len__(self):
        return check(lib().ccd_enc_size(self._h), "ccd_enc_size")

    def add(self, arch: CCHeader, bytes_nn: bytes, latents: Sequence[np.ndarray]) -> int:
        """Host latents (index 0 = finest grid, values in [-64, 63]); returns the slot."""
        arrs = [np.ascontiguousarray(a, dtype=np.int8) for a in latents]
        slot = check(lib().ccd_enc_add(self._h, C.byref(arch), bytes_nn, len(bytes_nn), ptr_array([a.ctypes.data for a in arrs]), 0), "ccd_enc_add")
        self._grid_shapes.append([a.shape[-2:] for a in arrs])
        return slot

    def add_device(self, arch: CCHeader, bytes_nn: bytes, latent_ptrs: Sequence[int], owner=None) -> int:
        """Latents that already sit on the device (int8 [h][w] per grid); they are read when run() executes."""
        slot = check(lib().ccd_enc_add(self._h, C.byref(arch), bytes_nn, len(bytes_nn), ptr_array(latent_ptrs), 1), "ccd_enc_add")
        self._note_grids(arch, len(latent_ptrs))
        self._keep(owner)  # (the decode batch whose device latents the slot reads at run())
        return slot

    def add_from_decode(self, batch: DecodeBatch, slot: int) -> int:
        """Re-encodes what `batch` decoded in `slot`: architecture, NN payload and the device latent grids are taken from the
        decode batch, nothing crosses PCIe.  The batch must have been run (and stay alive) before this handle runs."""
        h = batch.header(slot)
        ptrs = [lib().ccd_batch_latent(batch._h, slot, g) for g in range(h.n_grids)]
        return self.add_device(h, batch.network_bytes(slot), ptrs, owner=batch)

    def run(self, stream: int = 0):
        check(lib().ccd_enc_run(self._h, C.c_void_p(stream or None)), "ccd_enc_run")

    def wait(self, stream: int = 0):
        check(lib().ccd_enc_wait(self._h, C.c_void_p(stream or None)), "ccd_enc_wait")

    def measure(self, stream: int = 0, rate_map: bool = False):
        """Enqueues the rate meter for every slot (takes the place of a run in flight; wait() ends it)."""
        check(lib().ccd_enc_measure(self._h, C.c_void_p(stream or None), int(bool(rate_map))), "ccd_enc_measure")

    def rate(self, slot: int) -> SlotRate:
        """After measure() + wait().  A slot with a poisoned device latent comes back with its status set, not as an exception."""
        r = EncRate()
        rc = lib().ccd_enc_slot_rate(self._h, int(slot), C.byref(r))
        if rc < 0 and rc != r.status:
            raise CcdError(rc, "ccd_enc_slot_rate")
        n = r.n_grids
        return SlotRate(int(r.status), np.array(r.bits[:n], np.float64), np.array(r.sum_width[:n], np.uint64),
                        np.array(r.n_symbols[:n], np.int64), float(r.total_bits), int(r.n_bytes_nn), int(r.n_bytes_header))

    def rate_map(self, slot: int, grid: int) -> _DevArray:
        """Bits of every latent of a grid where measure(rate_map=True) left them (float32 [h][w], valid until the next
        measure / close)."""
        return self._grid_map("ccd_enc_slot_rate_map", slot, grid, "<f4")

    def measure_deltas(self, stream: int = 0):
        """measure() followed by the rate sensitivity launches: rate() as after measure(), and delta_map() of every grid."""
        check(lib().ccd_enc_measure_deltas(self._h, C.c_void_p(stream or None)), "ccd_enc_measure_deltas")

    def delta_map(self, slot: int, grid: int) -> _DevArray:
        """After measure_deltas() + wait(): float32 [2][h][w], the exact change of the slot's model bits if the latent at
        (y, x) alone were v - 1 (plane 0) or v + 1 (plane 1); +inf where that leaves [-64, 63].  Valid until the next measure /
        measure_deltas / close."""
        return self._grid_map("ccd_enc_slot_delta_map", slot, grid, "<f4", (2,))

    def measure_param_deltas(self, stream: int = 0, first: int = 0, count: int = -1, mode: int = 0):
        """measure() followed by the ARM parameter table's launches: rate() as after measure(), and
        param_deltas() of every slot for the ARM integers [first, first + count) in stream order (count < 0: all; clipped to
        each slot's param_count()).  mode 0 automatic, 1 generic, 2 incremental (refused where a slot cannot take it)."""
        check(lib().ccd_enc_measure_param_deltas(self._h, C.c_void_p(stream or None), int(first), int(count), int(mode)),
              "ccd_enc_measure_param_deltas")

    def param_count(self, slot: int) -> int:
        """Transmitted integers of the slot's ARM: groups 0 and 1 of writer.network_layout."""
        return check(lib().ccd_enc_slot_param_count(self._h, int(slot)), "ccd_enc_slot_param_count")

    def param_deltas(self, slot: int) -> ParamDeltas:
        """After measure_param_deltas() + wait(): per parameter and sign ([count][2], -1 first) the exact change of the slot's
        total model bits (float64, +inf where the integer would leave int32), of its sum of interval widths and the number of
        symbols whose width changed.  A slot with a latent outside the alphabet raises its status."""
        return self._table("ccd_enc_slot_param_deltas", slot)

    def _table(self, getter: str, slot: int) -> ParamDeltas:
        fn = getattr(lib(), getter)
        first, count = C.c_int(0), C.c_int(0)
        check(fn(self._h, int(slot), C.byref(first), C.byref(count), None, None, None), getter)
        bits = np.empty((count.value, 2), np.float64)
        sum_width, moved = np.empty((count.value, 2), np.int64), np.empty((count.value, 2), np.int64)
        check(fn(self._h, int(slot), None, None, bits.ctypes.data, sum_width.ctypes.data, moved.ctypes.data), getter)
        return ParamDeltas(first.value, bits, sum_width, moved)

    def measure_ifce_deltas(self, stream: int = 0, first: int = 0, count: int = -1, mode: int = 0):
        """measure() followed by the IFCE parameter table's launches: rate() as after measure(), and
        ifce_deltas() of every slot for the IFCE integers [first, first + count) in stream order (count < 0: all; clipped to each
        slot's ifce_count()).  Modes as measure_param_deltas.  A handle holds one table: param_deltas() refuses after this."""
        check(lib().ccd_enc_measure_ifce_deltas(self._h, C.c_void_p(stream or None), int(first), int(count), int(mode)),
              "ccd_enc_measure_ifce_deltas")

    def ifce_count(self, slot: int) -> int:
        """Transmitted integers of the slot's IFCE: groups 2 and 3 of writer.network_layout; 0 for a slot without IFCE."""
        return check(lib().ccd_enc_slot_ifce_count(self._h, int(slot)), "ccd_enc_slot_ifce_count")

    def ifce_deltas(self, slot: int) -> ParamDeltas:
        """After measure_ifce_deltas() + wait(): param_deltas()' three arrays for the IFCE integers; rows count from the first
        IFCE integer, so row r is values[param_count(slot) + first + r] of writer.network_values."""
        return self._table("ccd_enc_slot_ifce_deltas", slot)

    def slot_status(self, slot: int) -> Tuple[int, np.ndarray]:
        """(status, counters) after wait(): counters[1] payload words, [2] inverted runs begun by the coder, [3] resolved
        with a carry, [4] resolved without one (include/ccd.h)."""
        out = np.zeros(8, dtype=np.int32)
        return lib().ccd_enc_slot_status(self._h, int(slot), out.ctypes.data), out

    def bytes(self, slot: int) -> bytes:
        out = C.POINTER(C.c_uint8)()
        n = check(lib().ccd_enc_slot_bytes(self._h, int(slot), C.byref(out)), "ccd_enc_slot_bytes")
        try:
            return bytes(np.ctypeslib.as_array(out, shape=(n,)))
        finally:
            lib().ccd_free(out)

    def payload(self, slot: int) -> _DevArray:
        """The range-coded payload where the device wrote it (uint8, valid until the next run / close)."""
        ptr = C.c_void_p()
        n = check(lib().ccd_enc_slot_payload(self._h, int(slot), C.byref(ptr)), "ccd_enc_slot_payload")
        return _DevArray(ptr.value or 0, (n,), "|u1", self)


def payload_bound(n_symbols: int) -> int:
    return int(lib().ccd_enc_payload_bound(int(n_symbols)))
