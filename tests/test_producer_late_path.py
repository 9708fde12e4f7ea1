"""The producers' late path of the pipelined entropy kernel (ccd_entropy_pipe.hip, producer_grid, vector-ALU path): the window
builder's integer entry against window_left, and every producer instantiation at the smallest picture sizes that reach it,
on latents crafted to reach every case of the window builder (tests/producer_cases.py)."""
import os
import sys

import numpy as np
import pytest

import producer_cases as pc
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cool_chic_amd import DecodeBatch, _lib

    _lib.lib()
    return DecodeBatch


class _Stream:
    def __init__(self, oracle, fh, hdr_donor, nn, size):
        from cool_chic_amd import writer

        self.size = size
        self.fh = fh
        arch = writer.derive_arch(hdr_donor, img_size=size)
        assert writer.network_layout(arch) == writer.network_layout(hdr_donor)
        self.arch = arch
        self.latents = pc.crafted_latents(arch)
        self.stream = writer.encode_stream(writer.cc_header_bytes(arch), nn, self.latents, bitdepth=fh.bitdepth,
                                           frame_data_type=fh.frame_data_type)
        self.triple = oracle.split_stream(self.stream)[1][0][1][0]
        ref = oracle.decode_coolchic(*self.triple, stop_after_entropy=True)
        self.ref_latents = [np.array(a) for a in ref["latent"]]
        self.census = [pc.window_cases(np.array(ms)) for ms in ref["mu_scale_idx"]]
        self.planes = [np.array(p) for p in oracle.decode_video(self.stream)[0]["planes"]]


@pytest.fixture(scope="module")
def donor(oracle):
    from cool_chic_amd import writer

    bs, z, _ = load_golden("kodim14")
    (fh, ccs), = oracle.split_stream(bs)[1]
    hdr, nn, _ = ccs[0]
    return fh, writer.parse_cc_header(hdr), nn, np.array(z["cc0.nn_ints"])


@pytest.fixture(scope="module")
def streams(oracle, donor):
    """One stream per size of producer_cases.SIZES (kodim14's HOP networks, the crafted latents), with the oracle's latents,
    table indices and integer planes: built once, shared by the tests below."""
    fh, hdr, nn, _ = donor
    return {size: _Stream(oracle, fh, hdr, nn, size) for size in pc.SIZES}


def test_crafted_latents_reach_every_window_case(streams):
    """On the CPU, with the oracle's table indices: every grid that matters for a task size holds 14-symbol windows whose top
    symbol clamps at the low and at the high edge of the alphabet, windows that reach symbol 63 (the entry whose probability
    runs to 2^24), 62-symbol windows (scale index above 1280), and pixels at the smallest scale index; and the oracle decodes
    the crafted latents from the written stream.  40 x 260 has its first three grids on 8-, 4- and 2-pixel tasks."""
    s = streams[(40, 260)]
    assert [pc.task_pixels(s.arch.grid_h[g], s.arch.grid_w[g]) for g in range(3)] == [8, 4, 2]
    t = streams[(120, 100)]
    assert [pc.task_pixels(t.arch.grid_h[g], t.arch.grid_w[g]) for g in range(2)] == [4, 2]
    assert pc.task_pixels(260, 40) == 2 and pc.task_pixels(48, 256) == 8 and pc.task_pixels(56, 500) == 8
    for size, s in streams.items():
        for g, (a, b) in enumerate(zip(s.latents, s.ref_latents)):
            assert np.array_equal(a, b), (size, g)
        for g in range(3):
            c = s.census[g]
            print(size, "grid", g, c)
            for case in ("narrow", "wide", "top_clamped_low", "top_clamped_high", "reaches_63", "wide_reaches_63", "scale_0"):
                assert c[case] > 0, (size, g, case, c)
            assert c["min_scale"] == 0


def _check(b, slot, s):
    assert b.slot_status(slot) == 0
    for g, a in enumerate(s.ref_latents):
        assert np.array_equal(b.latent(slot, g), a), f"size {s.size} grid {g}"
    for p, (got, want) in enumerate(zip(b.planes(slot), s.planes)):
        assert got.shape == want.shape and np.array_equal(got.astype(np.uint16), want), f"size {s.size} plane {p}"


@pytest.mark.gpu
@pytest.mark.parametrize("size", list(pc.SIZES))
def test_producer_variants_on_crafted_latents(gpu, streams, size):
    """Latents of every grid and the integer planes bit for bit against the oracle, through the fixed-shape (HOP) instantiation
    of the pipelined kernel.  slot_stats tells which paths ran as far as the kernel counts them: grids streamed ([36]), symbols
    the decoder took outside its window, i.e. the rare path ([62]) and its full search ([63], the uniform-noise band), no int64
    redo ([39]); the window builder's own cases are not counted on the device - that the inputs hold them is the CPU test
    above."""
    s = streams[size]
    b = gpu(0)
    try:
        b.add(*s.triple, s.fh.bitdepth, s.fh.frame_data_type)
        b.run()
        b.wait()
        st = b.slot_stats(0)
        print(size, pc.SIZES[size], "streamed grids", st[36], "part batches", st[37], "rare", st[62], "searches", st[63])
        assert b.slot_kernels(0) & 1 and b.slot_kernels(0) & 32, b.slot_kernels(0)
        assert not b.slot_kernels(0) & 8
        _check(b, 0, s)
        assert st[39] == 0
        assert st[62] > 0 and st[63] > 0
        if size in ((48, 256), (56, 500)):
            assert st[36] >= 1, "no grid was streamed"
    finally:
        b.close()


@pytest.mark.gpu
def test_feature_checking_instantiation_on_crafted_latents(gpu, oracle, donor):
    """The second production instantiation (device check of the IFCE features, run-time ARM shape): synth.kodak24_wide_envelope's
    network on the 40 x 260 picture with the crafted latents."""
    from cool_chic_amd import writer

    fh, hdr, _, ints = donor
    hdr_w, nn_w, wide = pc.wide_envelope_network(writer.parse_cc_header(writer.cc_header_bytes(hdr)), ints)
    s = _Stream(oracle, fh, wide, nn_w, (40, 260))
    for g in range(3):
        assert s.census[g]["wide"] > 0 and s.census[g]["reaches_63"] > 0 and s.census[g]["top_clamped_low"] > 0, (g, s.census[g])
    b = gpu(0)
    try:
        b.add(*s.triple, fh.bitdepth, fh.frame_data_type)
        b.run()
        b.wait()
        print("kernels", b.slot_kernels(0), "pixels redone in int64", b.slot_stats(0)[39])
        assert b.slot_kernels(0) & 1 and b.slot_kernels(0) & 16 and not b.slot_kernels(0) & 8, b.slot_kernels(0)
        _check(b, 0, s)
    finally:
        b.close()


@pytest.mark.gpu
def test_integer_window_entry_equals_window_left(gpu):
    """window_left_d256 (what the producers and the pipelined kernel's sweep run: 256 (x - mu) from one integer subtraction, the
    reciprocal scaled by 2^-8) against window_left (what the generic kernel's sweep runs, the function every other kernel keeps
    calling): all 32768 mu indices x 127 symbols at scale indices 0, 1, 2, 1279, 1280, 1281, 2559, 2560 and every 64th - the
    scale indices of test_gpu_parity.py::test_laplace_boundaries_sweep, which holds both against libm.  Not one may differ.
    The whole domain (tools/cdf_sweep.py) was run once by hand: profiles/r07/cdf_sweep_window_d256.log."""
    from cool_chic_amd._lib import check, lib

    scales = sorted(set(list(range(0, 2561, 64)) + [0, 1, 2, 1279, 1280, 1281, 2559, 2560]))
    new = np.empty((32768, 127), dtype=np.uint32)
    old = np.empty((32768, 127), dtype=np.uint32)
    n_bad, first = 0, []
    for c in scales:
        check(lib().ccd_debug_laplace_sweep(0, 0, c, 1, new.ctypes.data), "ccd_debug_laplace_sweep")
        check(lib().ccd_debug_laplace_sweep(0, 1, c, 1, old.ctypes.data), "ccd_debug_laplace_sweep")
        bad = np.argwhere(new != old)
        n_bad += len(bad)
        first += [(c, int(m), int(k) - 63, int(new[m, k]), int(old[m, k])) for m, k in bad[:4]]
    assert n_bad == 0, f"{n_bad} boundaries differ, first (scale_idx, mu_idx, s, window_left_d256, window_left): {first[:8]}"
