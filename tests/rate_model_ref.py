"""Reference and inputs of tests/test_rate_model.py: the rate model (coolchic/component/core/arm.py:448-485) restated in PyTorch on
the CPU at a chosen precision, the per-symbol tolerance, and three seeded input families (float32 tensors, 1-D).

Truth is `reference(..., torch.float64)`: float32 inputs widen exactly, so the float64 result is the value of the formula AT the
float32 inputs to ~1e-16, nine digits below anything the tolerance can see."""
import functools
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_MIN = 2.0 ** -16     # no symbol costs more than 16 bits
SWITCH = -0.25         # the kernel's expm1 takes its Taylor series above this argument and exp2(t log2 e) - 1 below


@functools.lru_cache(maxsize=None)
def scale_table():
    """The 2561 float32 scales of the format (include/ccd_scale_table.inc), ascending: 0.0067 .. 148."""
    text = open(os.path.join(ROOT, "include", "ccd_scale_table.inc")).read()
    tab = np.array([int(t, 16) for t in re.findall(r"0x([0-9a-f]{8})u", text)], dtype=np.uint32).view(np.float32)
    assert tab.size == 2561
    return torch.from_numpy(tab.copy())


def reference(x, mu, scale, dtype):
    """(rate, p) of arm.py:448-485 evaluated in `dtype`; p is the probability BEFORE the 2^-16 clamp."""
    x, mu, scale = x.to(dtype), mu.to(dtype), scale.to(dtype)

    def cdf(t):
        d = t - mu
        return 0.5 - 0.5 * d.sign() * torch.expm1(-d.abs() / scale)

    p = cdf(x + 0.5) - cdf(x - 0.5)
    return -torch.log2(torch.clamp_min(p, P_MIN)), p


def cdf_arguments(x, mu, scale):
    """[2, n] float64: the two arguments -|x +- 0.5 - mu| / scale that the model hands to expm1."""
    x, mu, scale = x.double(), mu.double(), scale.double()
    return torch.stack([-(x + 0.5 - mu).abs() / scale, -(x - 0.5 - mu).abs() / scale])


def tolerance(want64, p64):
    """Bits per symbol: 2e-6 relative + 2e-6 + 3e-7 / p.  The last term is the formula's own float32 conditioning (p is a
    difference of two CDF values near 0.5 .. 1, each good to ~6e-8)."""
    return 2e-6 * want64.abs() + 2e-6 + 3e-7 / torch.clamp_min(p64, P_MIN)


def worst_ratio(got, want64, p64):
    """max over ALL symbols of |got - want64| / tolerance; a NaN in `got` gives inf."""
    r = (got.double() - want64).abs() / tolerance(want64, p64)
    return float(torch.nan_to_num(r, nan=float("inf")).max())


def family_a():
    """Decoder domain: every scale of the table x every mu fraction k / 256 x every offset x - floor(mu) in -8 .. 8
    (2561 * 256 * 17 = 11 145 472 symbols); the integer part of mu is seeded in [-40, 40)."""
    tab = scale_table()
    g = torch.Generator().manual_seed(0xA)
    n_s, n_f, n_o = tab.numel(), 256, 17
    shape = (n_s, n_f, n_o)
    ipart = torch.randint(-40, 40, shape, generator=g).float()
    frac = (torch.arange(n_f, dtype=torch.float32) / 256).view(1, n_f, 1)
    off = torch.arange(-8, 9, dtype=torch.float32).view(1, 1, n_o)
    mu = (ipart + frac).reshape(-1)                      # exact in float32: |mu| < 64 on the 1 / 256 grid
    x = (ipart + off).reshape(-1)
    scale = tab.view(n_s, 1, 1).expand(shape).reshape(-1)
    return x, mu, scale


def family_b():
    """The branch switch: 2^20 symbols, scale a random table entry, |d| = 0.25 scale (1 + k 2^-23) for k in -64 .. 64, d placed at
    x + 0.5 or x - 0.5 with either sign, so that one CDF argument of every symbol sits at -0.25 to within 64 ulps - exactly for
    scales >= 1, where mu = (x +- 0.5) - d is a float32; below that the rounding of mu (2^-26 next to 0.5) moves d by up to
    ~100 of ITS ulps, still on either side.  x is -1 or 0 in the first half (mu next to +-0.5: the finest grid) and any integer of
    [-64, 64) in the second (mu rounds at up to 2^-18: arguments spread to ~1e-3 around the switch for the narrowest scales)."""
    tab = scale_table()
    g = torch.Generator().manual_seed(0xB)
    n = 1 << 20
    scale = tab[torch.randint(0, tab.numel(), (n,), generator=g)]
    k = torch.randint(-64, 65, (n,), generator=g)
    d = (0.25 * scale.double() * (1 + k.double() * 2.0 ** -23)).float()
    d = torch.where(torch.randint(0, 2, (n,), generator=g) == 1, d, -d)
    half = torch.where(torch.randint(0, 2, (n,), generator=g) == 1, 0.5, -0.5)
    x = torch.cat([torch.randint(-1, 1, (n // 2,), generator=g), torch.randint(-64, 64, (n // 2,), generator=g)]).float()
    mu = ((x + half).double() - d.double()).float()
    return x, mu, scale


def family_c():
    """Beyond the table: 2^21 symbols, scale = 2^k (1 + u) for k in -20 .. 20, x an integer of [-64, 64), mu on the 1 / 256 grid
    over [-64, 64); half of the symbols steered to mu = x + N(0, 1) min(scale, 4): likely symbols at every scale."""
    g = torch.Generator().manual_seed(0xC)
    n = 1 << 21
    k = torch.randint(-20, 21, (n,), generator=g)
    scale = (torch.exp2(k.double()) * (1 + torch.rand(n, generator=g).double())).float()
    x = torch.randint(-64, 64, (n,), generator=g).float()
    mu = torch.randint(0, 128 * 256, (n,), generator=g).float() / 256 - 64
    steer = (x.double() + torch.randn(n, generator=g).double() * torch.clamp_max(scale.double(), 4.0)).float()
    mu = torch.where(torch.arange(n) % 2 == 0, steer, mu)
    return x, mu, scale


FAMILIES = {"A": family_a, "B": family_b, "C": family_c}


@functools.lru_cache(maxsize=None)
def family(name):
    """(x, mu, scale, want64, p64) of one family, computed once per process and shared: treat as read-only."""
    x, mu, scale = FAMILIES[name]()
    want64, p64 = reference(x, mu, scale, torch.float64)
    return x, mu, scale, want64, p64
