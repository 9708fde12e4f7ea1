"""The rate model (ccd_rate.hip: ccd_compute_rate, compute_rate, total_rate_bits) against the formula in float64, on every launch
path, at every alignment, with NaN, and at the wrapper's edges.

Truth is rate_model_ref.reference(..., float64) on the float32 inputs; the tolerance per symbol is the project's own (2e-6 relative
+ 2e-6 bits + 3e-7 / p bits), taken against that truth and over every symbol.  The launch-path, alignment
and NaN tests compare the device with itself bit for bit: one plain aligned launch, which the accuracy test anchors to the truth,
is the expectation for every other way the same values can reach the two kernels."""
import ctypes as C
import math

import numpy as np
import pytest

import rate_model_ref as R

ERR_ARG = -7
N_BASE = 1 << 16
# whole 4-symbol groups handed to rate_kernel_v4 (blocks = ceil(n4 / 512) up to 2048, two groups per lane and loop iteration):
# 1 / 255: part of one workgroup in the remainder; 256: all its lanes in the remainder; 257: one lane in the loop, the others in the
# remainder; 511 / 512: all lanes in the loop (but one); 513: a second workgroup.  N4_BIG reaches the cap of 2048 workgroups
# (stride 2^19): every lane runs the loop twice, the first 77 a third time, all the others take the remainder behind the loop.
N4_SMALL = (1, 255, 256, 257, 511, 512, 513)
N4_BIG = 2048 * 512 * 2 + 2048 * 256 + 77
GUARD = 64
SENTINEL = 0x7FC5A5A5  # as int32 bits: a quiet NaN with a payload no arithmetic produces


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_float32_reference_is_within_the_tolerance_of_the_truth(name):
    """Keeps the tolerance honest without any kernel: the reference formula in float32 stays within it of the float64 truth on
    every symbol of the three families.  Worst |error| / tolerance, measured: A 0.425, B 0.292, C 0.424 (an emulation of the
    kernel's arithmetic with exact exp2 / log2 / reciprocal: 0.425, 0.376, 0.431).
    No family is degenerate: > 1000 symbols with p > 0.5, > 1000 CDF arguments on each side of the kernel's switch at -0.25, and
    > 1000 symbols on the 2^-16 clamp in A and C.  B cannot reach the clamp: one CDF value of each of its symbols sits at
    0.5 -+ 0.5 expm1(-0.25) = 0.61 or 0.39 and the other one 1 / scale further along, so p >= 0.5 e^-0.25 (1 - e^(-1 / scale)) =
    2.6e-3 at the table's largest scale (148.4).  That bound is asserted for B in place of the clamp count; B's symbols are
    instead all next to the switch: > 2^19 of its arguments within 64 * 2^-25 of -0.25."""
    import torch

    x, mu, scale, want64, p64 = R.family(name)
    assert x.dtype == mu.dtype == scale.dtype == torch.float32 and want64.dtype == p64.dtype == torch.float64
    assert x.numel() == {"A": 2561 * 256 * 17, "B": 1 << 20, "C": 1 << 21}[name]
    got32, _ = R.reference(x, mu, scale, torch.float32)
    ratio = R.worst_ratio(got32, want64, p64)
    print(f"family {name}: float32 reference, worst |error| / tolerance = {ratio:.3f}")
    assert ratio <= 1.0
    assert int((p64 > 0.5).sum()) > 1000
    args = R.cdf_arguments(x, mu, scale)
    assert int((args > R.SWITCH).sum()) > 1000 and int((args < R.SWITCH).sum()) > 1000
    if name == "B":
        s_max = float(R.scale_table().max())
        assert float(p64.min()) >= 0.999 * 0.5 * math.exp(-0.25) * (1 - math.exp(-1 / s_max)) > R.P_MIN
        near = (args - R.SWITCH).abs() <= 64 * 2.0 ** -25
        assert int((near & (args > R.SWITCH)).sum()) > 1 << 17 and int((near & (args < R.SWITCH)).sum()) > 1 << 17
        assert int(near.sum()) > 1 << 19
    else:
        assert int((p64 < R.P_MIN).sum()) > 1000
    if name == "A":  # every scale, every fraction, every offset
        assert torch.equal(scale.unique(), R.scale_table())
        assert torch.equal(((mu - mu.floor()) * 256).unique(), torch.arange(256.0))
        assert torch.equal((x - mu.floor()).unique(), torch.arange(-8.0, 9.0))


def test_abi_argument_errors_need_no_device():
    """ccd_compute_rate refuses a NULL x, mu or scale, n < 0 and two NULL outputs with CCD_ERR_ARG before it touches a device
    (host-side part of the C ABI, like ccd_png_bound)."""
    from cool_chic_amd import _lib

    L = _lib.lib()
    buf = (C.c_float * 8)()  # never dereferenced: every call below fails its argument check
    p = C.addressof(buf)
    tot = C.c_double(1.5)
    for x, mu, scale, n, rate, total in ((None, p, p, 4, p, None), (p, None, p, 4, p, None), (p, p, None, 4, p, None),
                                         (p, p, p, -1, p, None), (p, p, p, -1, None, C.addressof(tot)), (p, p, p, 4, None, None),
                                         (p, p, p, 0, None, None), (None, None, None, 0, None, None)):
        assert L.ccd_compute_rate(0, None, x, mu, scale, n, rate, total) == ERR_ARG
    assert tot.value == 1.5 and not any(buf)


def _no_library(monkeypatch):
    from cool_chic_amd.component.core import arm

    def boom():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(arm, "lib", boom)
    return arm


def test_host_tensors_are_refused(monkeypatch):
    import torch

    arm = _no_library(monkeypatch)
    t = torch.ones(8)
    for fn in (arm.compute_rate, arm.total_rate_bits):
        with pytest.raises(ValueError):
            fn(t, t, t)
        with pytest.raises(ValueError):
            fn(t.double(), t.double(), t.double())


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cool_chic_amd import _lib

    return _lib.lib()


def _bits(t):
    import torch

    return t.view(torch.int32)


def _launch(L, x, mu, scale, n, rate=None, total=None):
    """ccd_compute_rate through ctypes on torch's current stream; x / mu / scale / rate / total: device addresses (int) or None."""
    import torch

    stream = torch.cuda.current_stream().cuda_stream
    code = L.ccd_compute_rate(0, C.c_void_p(stream or None), C.c_void_p(x), C.c_void_p(mu), C.c_void_p(scale), n,
                              C.c_void_p(rate), C.c_void_p(total))
    assert code == 0, code


def _guarded(n, front=0):
    """float32 [front + n + GUARD] on the device, every element the sentinel."""
    import torch

    return torch.full((front + n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def _only_sentinel(t):
    return bool((_bits(t) == SENTINEL).all())


@pytest.fixture(scope="module")
def base(gpu):
    """2^16 symbols drawn (seeded) from family A, on the device, with the device's rates from ONE plain aligned launch: the
    expectation of every bit-for-bit test below.  Anchored to the truth here too (and at full size by the accuracy test)."""
    import torch

    x, mu, scale, want64, p64 = R.family("A")
    idx = torch.randperm(x.numel(), generator=torch.Generator().manual_seed(5))[:N_BASE]
    dev = [t[idx].cuda() for t in (x, mu, scale)]
    rate = _guarded(N_BASE)
    _launch(gpu, *(t.data_ptr() for t in dev), N_BASE, rate.data_ptr())
    assert _only_sentinel(rate[N_BASE:])
    rate = rate[:N_BASE].clone()
    assert R.worst_ratio(rate.cpu(), want64[idx], p64[idx]) <= 1.0
    return dev[0], dev[1], dev[2], rate


def _tiled(t, n):
    return t.repeat(-(-n // t.numel()))[:n].contiguous()


@pytest.fixture(scope="module")
def big(base):
    """The base pattern tiled to 4 * N4_BIG + 3 symbols (10.5 M, 42 MB per array), shared by the launch-path and totals tests."""
    n = 4 * N4_BIG + 3
    return tuple(_tiled(t, n) for t in base)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_device_is_within_the_tolerance_of_the_truth(gpu, name):
    """compute_rate against the float64 truth on every symbol of a family, 0 <= rate <= 16, and the share of symbols at exactly 16.0
    against the truth's clamped share: they may differ by the symbols whose p is within 2e-7 (float32 noise of a CDF difference) of
    2^-16, whichever side those fall on.  Worst |error| / tolerance measured on the MI355X: A 0.425, B 0.405, C 0.431 (DESIGN.md
    section 4.8, which also says what this tolerance cannot see: a degree-5 series reaches 0.98 on B and still passes)."""
    from cool_chic_amd.component.core.arm import compute_rate

    x, mu, scale, want64, p64 = R.family(name)
    got = compute_rate(x.cuda(), mu.cuda(), scale.cuda()).cpu()
    ratio = R.worst_ratio(got, want64, p64)
    print(f"family {name}: device, worst |error| / tolerance = {ratio:.3f}")
    if ratio > 1.0:
        err = (got.double() - want64).abs() / R.tolerance(want64, p64)
        for i in err.argsort(descending=True)[:5].tolist():
            print(f"  x {float(x[i])!r} mu {float(mu[i])!r} scale {float(scale[i])!r} got {float(got[i])!r} want {float(want64[i])!r} "
                  f"p {float(p64[i])!r} args {R.cdf_arguments(x[i:i + 1], mu[i:i + 1], scale[i:i + 1]).flatten().tolist()}")
    assert ratio <= 1.0
    assert float(got.min()) >= 0.0 and float(got.max()) <= 16.0
    n = x.numel()
    edge = int(((p64 - R.P_MIN).abs() <= 2e-7).sum())
    print(f"family {name}: {int((got == 16.0).sum())} symbols at 16.0, {int((p64 < R.P_MIN).sum())} clamped in the truth, {edge} on the edge of {n}")
    assert abs(int((got == 16.0).sum()) - int((p64 < R.P_MIN).sum())) <= edge


def _check_path(L, src, want, n):
    """One launch over the first n symbols of src = (x, mu, scale): the bits of want[:n], nothing behind them."""
    import torch

    rate = _guarded(n)
    _launch(L, src[0].data_ptr(), src[1].data_ptr(), src[2].data_ptr(), n, rate.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(_bits(rate[:n]), _bits(want[:n])), f"n = {n}: bits differ from the plain launch"
    assert _only_sentinel(rate[n:]), f"n = {n}: a write behind rate[n - 1]"


@pytest.mark.gpu
@pytest.mark.parametrize("n4", N4_SMALL)
def test_launch_paths_give_the_same_bits(gpu, base, n4):
    """The base pattern (tiled where longer) through n = 4 n4 + r symbols, r = 0 .. 3: every way the lanes of rate_kernel_v4 split
    between loop and remainder, with the scalar tail behind them, gives the bits of the plain launch and leaves the 64 floats behind
    rate[n - 1] alone."""
    n_max = 4 * n4 + 3
    src = tuple(_tiled(t, n_max) for t in base)
    for r in range(4):
        _check_path(gpu, src[:3], src[3], 4 * n4 + r)


@pytest.mark.gpu
def test_capped_grid_gives_the_same_bits(gpu, big):
    """10.5 M symbols: 2048 workgroups, two and three loop iterations per lane, then the remainder; r = 0 and r = 3."""
    for r in (0, 3):
        _check_path(gpu, big[:3], big[3], 4 * N4_BIG + r)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["x", "mu", "scale", "rate", "all"])
def test_every_alignment_gives_the_same_bits(gpu, base, which):
    """n = 4099 with one array (or all four) starting 1, 2 or 3 floats off a 16-byte boundary and the others aligned: the scalar
    kernel's bits are those of the aligned call on the same values, and the floats on either side of rate[0 .. n) stay as they were."""
    import torch

    n = 4099
    for off in (1, 2, 3):
        ptrs = []
        keep = []
        for name, t in zip(("x", "mu", "scale"), base[:3]):
            o = off if which in (name, "all") else 0
            buf = torch.zeros(o + n, device="cuda")
            buf[o:] = t[:n]
            keep.append(buf)
            assert buf.data_ptr() % 16 == 0
            ptrs.append(buf.data_ptr() + 4 * o)
        o = off if which in ("rate", "all") else 0
        rate = _guarded(n, front=o)
        assert rate.data_ptr() % 16 == 0
        _launch(gpu, *ptrs, n, rate.data_ptr() + 4 * o)
        torch.cuda.synchronize()
        assert torch.equal(_bits(rate[o:o + n]), _bits(base[3][:n])), (which, off)
        assert _only_sentinel(rate[:o]) and _only_sentinel(rate[o + n:]), (which, off)


def _sum_bound(rate, n):
    """(math.fsum of the device's own rates widened to float64, n 2^-53 sum): any order of adding n non-negative doubles is within
    that bound of the exact sum, and the order of the kernel's atomic adds is not fixed."""
    s = math.fsum(rate.double().cpu().tolist())
    return s, n * 2.0 ** -53 * s


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 7, 4099, 4 * N4_BIG + 3])
def test_totals(gpu, base, big, n):
    """total_bits alone, rate and total_bits in one call, a total that held 1e300 before the call, the same double reused by two
    calls in a row, and n = 0 (total 0.0, rate untouched)."""
    import torch

    src = big if n > N_BASE else base
    ptrs = [t.data_ptr() for t in src[:3]]
    want = src[3][:n]
    s, bound = _sum_bound(want, n)
    total = torch.full((1 + GUARD,), 1e300, dtype=torch.float64, device="cuda")
    # total alone, over a stale value; then the same double again
    for _ in range(2):
        _launch(gpu, *ptrs, n, None, total.data_ptr())
        got = float(total[0])
        print(f"n = {n}: total {got!r}, fsum {s!r}, bound {bound!r}")
        assert abs(got - s) <= bound
        assert bool((total[1:] == 1e300).all())
    # both outputs in one call
    total[0] = -1e300
    rate = _guarded(n)
    _launch(gpu, *ptrs, n, rate.data_ptr(), total.data_ptr())
    assert abs(float(total[0]) - s) <= bound
    assert torch.equal(_bits(rate[:n]), _bits(want)) and _only_sentinel(rate[n:])
    assert bool((total[1:] == 1e300).all())
    if n == 0:
        assert float(total[0]) == 0.0 and s == 0.0


@pytest.mark.gpu
def test_wrapper_views_streams_and_shapes(gpu, base):
    """compute_rate / total_rate_bits on non-contiguous inputs (a transposed view, a [::2] slice, a stride-0 expand for scale) give
    the bits of the contiguous copies; a side stream gives the same bits; the shape is kept."""
    import torch

    from cool_chic_amd.component.core.arm import compute_rate, total_rate_bits

    x, mu, scale, rate = base
    # transposed views
    xt, mt, st = (t[:64 * 65].view(64, 65).t() for t in (x, mu, scale))
    assert not xt.is_contiguous()
    got = compute_rate(xt, mt, st)
    assert got.shape == (65, 64)
    assert torch.equal(_bits(got), _bits(rate[:64 * 65].view(64, 65).t().contiguous()))
    # [::2] slices (one of them against contiguous partners)
    got = compute_rate(x[::2], mu[::2], scale[::2])
    assert got.shape == (N_BASE // 2,) and torch.equal(_bits(got), _bits(rate[::2].contiguous()))
    got = compute_rate(x[:N_BASE // 2], mu[::2], scale[:N_BASE // 2])
    assert torch.equal(_bits(got), _bits(compute_rate(x[:N_BASE // 2], mu[::2].contiguous(), scale[:N_BASE // 2])))
    # stride-0 expand for scale; a 3-D shape
    s0 = scale[777].expand(3, 5, 1367)
    assert s0.stride() == (0, 0, 0)
    x3, m3 = x[:3 * 5 * 1367].view(3, 5, 1367), mu[:3 * 5 * 1367].view(3, 5, 1367)
    got = compute_rate(x3, m3, s0)
    want = compute_rate(x3.contiguous(), m3.contiguous(), s0.contiguous())
    assert got.shape == (3, 5, 1367) and torch.equal(_bits(got), _bits(want))
    assert R.worst_ratio(got.cpu(), *R.reference(x3.cpu(), m3.cpu(), s0.cpu(), torch.float64)) <= 1.0
    s, bound = _sum_bound(want.flatten(), want.numel())
    assert abs(total_rate_bits(x3, m3, s0) - s) <= bound
    s, bound = _sum_bound(rate[::2], N_BASE // 2)
    assert abs(total_rate_bits(x[::2], mu[::2], scale[::2]) - s) <= bound
    # a side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = compute_rate(x, mu, scale)
        tot = total_rate_bits(x, mu, scale)
    side.synchronize()
    assert torch.equal(_bits(got), _bits(rate))
    s, bound = _sum_bound(rate, N_BASE)
    assert abs(tot - s) <= bound
    # nothing to do: an empty tensor keeps its shape, the total is 0
    e = torch.empty(0, 3, device="cuda")
    assert compute_rate(e, e, e).shape == (0, 3) and total_rate_bits(e, e, e) == 0.0


@pytest.mark.gpu
def test_wrapper_refuses_what_the_kernel_cannot_read(gpu, base, monkeypatch):
    """Both entry points raise ValueError BEFORE any library call for float64 or integer inputs, unequal shapes, tensors on different
    devices and a mixture of host and device tensors: the kernel would reinterpret the former and read past the end of a shorter
    tensor.  (The library is replaced by a stub that fails the test if it is reached.)"""
    import torch

    arm = _no_library(monkeypatch)
    x, mu, scale = (t[:4096] for t in base[:3])
    bad = [(x.double(), mu.double(), scale.double()), (x.double(), mu, scale), (x, mu.double(), scale), (x, mu, scale.double()),
           (x.int(), mu.int(), scale.int()), (x, mu, scale.long()), (x.half(), mu.half(), scale.half()),
           (x, mu[:4095], scale), (x, mu, scale[:1]), (x[:100], mu, scale), (x.view(64, 64), mu, scale), (x, mu, scale[0]),
           (x.cpu(), mu, scale), (x, mu.cpu(), scale), (x, mu, scale.cpu()), (x.cpu(), mu.cpu(), scale)]
    if torch.cuda.device_count() > 1:
        bad += [(x, mu.to("cuda:1"), scale), (x, mu, scale.to("cuda:1")), (x.to("cuda:1"), mu, scale)]
    for fn in (arm.compute_rate, arm.total_rate_bits):
        for args in bad:
            with pytest.raises(ValueError):
                fn(*args)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["vector", "scalar"])
def test_nan_in_gives_nan_out(gpu, base, kernel):
    """A NaN (either sign, quiet, with a payload) in x, in mu or in scale gives NaN at exactly those symbols - not the 16 bits of the
    clamp - in the vector kernel and in the scalar one (the tail behind the last group of four; everything when an array is
    unaligned); the finite neighbours keep their bits; total_bits is NaN exactly when a NaN is present."""
    import torch

    n = 4099  # 1024 groups of four in the vector kernel + 3 symbols in the scalar tail; all scalar when x is unaligned
    off = 1 if kernel == "scalar" else 0
    clean = [t[:n].clone() for t in base[:3]]
    nans = torch.tensor([0x7FC00000, 0xFFC00000 - (1 << 32), 0x7FC12345, 0x7F800001], dtype=torch.int32, device="cuda").view(torch.float32)
    # (array, position): every lane slot of a group, first and last group, a wave's last lane, the tail
    hits = {0: [0, 5, 1023, 4095, 4096], 1: [2, 255, 2048, 4094, 4097], 2: [3, 256, 257, 3001, 4098]}
    tail_only = {0: [4096], 1: [4097], 2: [4098]}
    vec_only = {0: [1], 1: [514], 2: [4095]}

    def run(places):
        # x alone carries the offset: one unaligned array sends everything to the scalar kernel
        src = [torch.zeros((off if a == 0 else 0) + n, device="cuda") for a in range(3)]
        mask = torch.zeros(n, dtype=torch.bool, device="cuda")
        for a in range(3):
            o = src[a].numel() - n
            src[a][o:] = clean[a]
            for j, i in enumerate(places.get(a, [])):
                src[a][o + i] = nans[(a + j) % 4]
                mask[i] = True
        ptrs = [src[0].data_ptr() + 4 * off, src[1].data_ptr(), src[2].data_ptr()]
        assert ptrs[0] % 16 == 4 * off and ptrs[1] % 16 == 0 and ptrs[2] % 16 == 0
        rate = _guarded(n)
        total = torch.full((1,), 1e300, dtype=torch.float64, device="cuda")
        _launch(gpu, *ptrs, n, rate.data_ptr(), total.data_ptr())
        torch.cuda.synchronize()
        assert _only_sentinel(rate[n:])
        return rate[:n], mask, float(total[0])

    want = base[3][:n]
    got, mask, tot = run({})
    assert not bool(mask.any()) and torch.equal(_bits(got), _bits(want)) and math.isfinite(tot)
    for places in (hits, tail_only, vec_only):
        got, mask, tot = run(places)
        assert int(mask.sum()) == sum(len(v) for v in places.values())
        bad = (torch.isnan(got) != mask).nonzero().flatten().tolist()
        assert not bad, f"{kernel} kernel: NaN expected at exactly the poisoned symbols; wrong at {bad}: {got[bad].tolist()}"
        assert torch.equal(_bits(got[~mask]), _bits(want[~mask])), "a finite neighbour changed"
        assert math.isnan(tot), f"total {tot!r} with {int(mask.sum())} NaN symbols"
