"""The producers' output tail of the pipelined entropy kernel (ccd_entropy_pipe.hip, producer_grid, vector-ALU path): on 8- and
4-pixel tasks the output layer runs on the activations each lane holds and is summed over the pixel's lane group, and the
pixel's own lanes build its window from the indices every one of them then has; 2-pixel tasks keep the exchange through the
activation tile.  Latents of every grid and the integer planes bit for bit against the CPU oracle, on networks that make a wrong
sum visible (tests/output_tail_cases.py) and on the crafted latents of tests/producer_cases.py through both shapes of
instantiation."""
import numpy as np
import pytest

import output_tail_cases as otc
import producer_cases as pc


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cool_chic_amd import DecodeBatch, _lib

    _lib.lib()
    return DecodeBatch


def test_exposed_unit_moves_the_indices_on_every_task_size(oracle):
    """On the CPU, from the oracle's table indices: the first three grids of every network run 8-, 4- and 2-pixel tasks; taking
    the exposed unit's output weights away, and doubling them (one extra copy of the unit in the sum over the lanes), each
    changes the (mu, scale) indices of at least a quarter of the pixels on every one of those grids; mu is nowhere saturated
    on more than half of a grid (a saturated index hides a wrong sum); and the oracle decodes the crafted latents."""
    for shape in otc.SHAPES:
        c = otc.case(oracle, shape)
        assert [pc.task_pixels(c.arch.grid_h[g], c.arch.grid_w[g]) for g in range(3)] == [8, 4, 2], c.name
        for a, b in zip(pc.crafted_latents(c.arch), c.latents):
            assert np.array_equal(a, b), c.name
        for g in range(3):
            n = len(c.mu_scale_idx[g])
            for other in (c.control_idx[g], c.doubled_idx[g]):
                changed = int((c.mu_scale_idx[g] != other).any(axis=1).sum())
                assert 4 * changed >= n, (c.name, g, changed, n)
            saturated = int(np.isin(c.mu_scale_idx[g][:, 0], (0, 32767)).sum())
            assert 2 * saturated <= n, (c.name, g, saturated, n)


def test_sizes_hold_tasks_with_pixels_missing():
    """40 x 260 (8-pixel tasks, longest step 27) and 260 x 40 (2-pixel tasks, steps of up to 4 at the ramps: 1 and 3) end steps in
    tasks with fewer pixels than lane groups: lanes of pixels that do not exist take part in the reduction."""
    assert pc.task_pixels(40, 260) == 8 and min(40, (260 - 1) // 10 + 1) % 8 != 0
    assert pc.task_pixels(20, 130) == 4 and min(20, (130 - 1) // 10 + 1) % 4 != 0
    assert pc.task_pixels(260, 40) == 2
    assert (40, 260) in pc.SIZES and (260, 40) in pc.SIZES


def _decode_and_check(gpu, triple, fh, latents, planes, what):
    b = gpu(0)
    try:
        b.add(*triple, fh.bitdepth, fh.frame_data_type)
        b.run()
        b.wait()
        kernels = b.slot_kernels(0)
        assert b.slot_status(0) == 0, what
        for g, a in enumerate(latents):
            assert np.array_equal(b.latent(0, g), a), f"{what} grid {g}"
        for p, (got, want) in enumerate(zip(b.planes(0), planes)):
            assert got.shape == want.shape and np.array_equal(got.astype(np.uint16), want), f"{what} plane {p}"
        return kernels
    finally:
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fixed", [True, False], ids=["fixed_shape", "runtime_shape"])
@pytest.mark.parametrize("size", list(pc.SIZES))
def test_crafted_latents_through_both_instantiations(gpu, oracle, monkeypatch, size, fixed):
    """Every size of producer_cases.SIZES (8-, 4- and 2-pixel tasks, streamed bodies, steps that end in short tasks, every case
    of the window builder) through the compile-time-shape instantiation and, with CCD_FIXED_SHAPE=0, the run-time-shape one."""
    if not fixed:
        monkeypatch.setenv("CCD_FIXED_SHAPE", "0")
    s = otc.crafted(oracle, size)
    kernels = _decode_and_check(gpu, s.triple, s.fh, s.latents, s.planes, f"size {size}")
    assert kernels & 1 and bool(kernels & 32) == fixed and not kernels & 8, kernels


@pytest.mark.gpu
@pytest.mark.parametrize("shape", otc.SHAPES, ids=[otc.name_of(s) for s in otc.SHAPES])
def test_exposed_last_unit(gpu, oracle, shape):
    """The networks of output_tail_cases at 32 x 320: 0, 1 and 2 hidden layers, dim 20, 19, 22, 6, 30 and 64; every one up to
    32 inputs through the pipelined kernel, the compile-time shape for 14 + 6 with two hidden layers only."""
    c = otc.case(oracle, shape)
    kernels = _decode_and_check(gpu, c.triple, c.fh, c.latents, c.planes, c.name)
    print(c.name, "kernels", kernels)
    if shape[0] + shape[1] <= 32:  # the pipelined kernel (bit 0) with the ARM on the vector ALU (bit 3 clear)
        assert kernels & 1 and not kernels & 8, (c.name, kernels)
    else:  # the generic kernel
        assert not kernels & 1, (c.name, kernels)
    assert bool(kernels & 32) == (shape == (14, 6, 2)), (c.name, kernels)


@pytest.mark.gpu
def test_exposed_last_unit_runtime_shape(gpu, oracle, monkeypatch):
    """The 14 + 6 network with two hidden layers again, through the run-time-shape instantiation."""
    monkeypatch.setenv("CCD_FIXED_SHAPE", "0")
    c = otc.case(oracle, (14, 6, 2))
    kernels = _decode_and_check(gpu, c.triple, c.fh, c.latents, c.planes, c.name)
    assert kernels & 1 and not kernels & 32, kernels
