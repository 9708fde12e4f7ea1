"""EncodeBatch: range-encodes the latents of many cool-chics on one MI355X (wraps the ccd_enc_* C ABI).

The bytes are those of writer.encode_coolchic (cool-chic header + NN payload + range-coded latents,
bitstream/encode.py:83-92); the contexts of every pixel are evaluated at once and one wave per slot runs the range
encoder's interval chain."""
import ctypes as C
from typing import List, Sequence, Tuple

import numpy as np

from ._lib import CCHeader, check, lib
from .batch import DecodeBatch, _DevArray


class EncodeBatch:
    """One slot per cool-chic; run() encodes all of them in the same two launches."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        check(lib().ccd_enc_create(int(device), C.byref(self._h)), "ccd_enc_create")
        self.device = int(device)
        self._owners: List[object] = []  # decode batches whose device latents the slots read at run()

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().ccd_enc_destroy(self._h)
            self._h = C.c_void_p()
            self._owners = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return check(lib().ccd_enc_size(self._h), "ccd_enc_size")

    def add(self, arch: CCHeader, bytes_nn: bytes, latents: Sequence[np.ndarray]) -> int:
        """Host latents (index 0 = finest grid, values in [-64, 63]); returns the slot."""
        arrs = [np.ascontiguousarray(a, dtype=np.int8) for a in latents]
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        return check(lib().ccd_enc_add(self._h, C.byref(arch), bytes_nn, len(bytes_nn), ptrs, 0), "ccd_enc_add")

    def add_device(self, arch: CCHeader, bytes_nn: bytes, latent_ptrs: Sequence[int], owner=None) -> int:
        """Latents that already sit on the device (int8 [h][w] per grid); they are read when run() executes."""
        ptrs = (C.c_void_p * len(latent_ptrs))(*[int(p) for p in latent_ptrs])
        slot = check(lib().ccd_enc_add(self._h, C.byref(arch), bytes_nn, len(bytes_nn), ptrs, 1), "ccd_enc_add")
        if owner is not None:
            self._owners.append(owner)
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
