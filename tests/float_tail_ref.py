"""Plain references for the tail of the float path, independent of the oracle's C (tests/test_float_tail.py):

nearest     F.interpolate(mode="nearest", size=...) on the CPU: word-exact (a gather).
interp      F.interpolate(mode="bilinear" | "bicubic", align_corners=False) on FLOAT64 input.  A float32 evaluation is not
            word-equal to another one (torch's own float32 kernel differs from the oracle in most words); what bounds a correct one
            is the float32 source coordinate, so the bar is MEASURED per case against the reference: `interp_bar`.
noise       the Park-Miller / Box-Muller loop in plain CPython `math` (noise.py:17-54 of the reference decoder), and the x2 bicubic
            chain of fixed_upsampling in float64.
planes      the literal chain of decode.py:191-206 in torch float32: exact.

The bar of an interpolated result `got` against the float64 reference `ref64` of the same input x:

    |got - ref64| <= 2 * max|F.interpolate(x as float32) - ref64| + FLOOR_ULPS * 2^-23 * max|x|

* the measured term is torch's own float32 kernel's distance from float64 on this very input: the cost of a float32 source
  coordinate and float32 coefficients at this scale;
* the factor 2: another evaluation order of the same float32 coordinates may land on the other side of the float64 value;
* the floor covers the cases where that measured term is rounding noise alone (tiny grids, exactly representable scales) and a
  different summation order can exceed twice of it.  A separable bicubic evaluation takes 4 products and 3 sums per axis, 8
  roundings of relative size 2^-24 on a path from an input to the output, each acting on partial sums bounded by
  (sum |w_x|) (sum |w_y|) max|x|.  With A = -0.75 the sum of |w| over the four taps is largest at t = 1/2:
  2 (0.59375 + 0.09375) = 1.375, squared 1.890625.  8 * 2^-24 * 1.890625 max|x| = 7.5625 * 2^-23 max|x|: FLOOR_ULPS = 8 units
  of 2^-23 max|x| (an ulp of the largest input magnitude, at most).  The bilinear kernel (2 taps, sum |w| = 1) is covered by the
  same floor.  A wrong tap, index or coefficient gives errors of 1e-2 and more."""
import math

import numpy as np

FLOOR_ULPS = 8.0
SIGMA_W = 1.375  # sum |w| of the bicubic kernel (A = -0.75) at t = 1/2, its maximum


def bicubic_weights(t, A=-0.75):
    x0, x1, x2, x3 = t + 1.0, t, 1.0 - t, 2.0 - t
    return (((A * x0 - 5 * A) * x0 + 8 * A) * x0 - 4 * A, ((A + 2) * x1 - (A + 3)) * x1 * x1 + 1,
            ((A + 2) * x2 - (A + 3)) * x2 * x2 + 1, ((A * x3 - 5 * A) * x3 + 8 * A) * x3 - 4 * A)


# ---- nearest ---------------------------------------------------------------------------------------------------------
def nearest(x, size):
    import torch
    import torch.nn.functional as F

    return F.interpolate(torch.from_numpy(np.ascontiguousarray(x))[None], size=tuple(size), mode="nearest")[0].numpy()


def nearest_index(n_in, n_out):
    """numpy restatement of nearest_src (ccd_float.hip / cc_oracle.c): the source index of every destination index."""
    dst = np.arange(n_out)
    if n_in == n_out:
        return dst
    if n_out == 2 * n_in:
        return dst >> 1
    scale = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(dst.astype(np.float32) * scale).astype(np.int64), n_in - 1)


def nearest_index_torch(n_in, n_out):
    import torch
    import torch.nn.functional as F

    return F.interpolate(torch.arange(n_in, dtype=torch.float32)[None, None], size=n_out, mode="nearest")[0, 0].numpy().astype(np.int64)


# ---- bilinear / bicubic ----------------------------------------------------------------------------------------------
def _interp(x, size, mode, dtype):
    import torch
    import torch.nn.functional as F

    t = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)[None]
    return F.interpolate(t, size=tuple(size), mode=mode, align_corners=False)[0].numpy()


def interp64(x, size, mode):
    return _interp(x, size, mode, __import__("torch").float64)


def interp_bar(x, size, mode, ref64=None):
    """(bar, measured): the bar of the module docstring for a float32 evaluation of this resize of x, and its measured term."""
    ref64 = interp64(x, size, mode) if ref64 is None else ref64
    measured = float(np.abs(_interp(x, size, mode, __import__("torch").float32).astype(np.float64) - ref64).max())
    return 2.0 * measured + FLOOR_ULPS * 2.0 ** -23 * float(np.abs(x).max()), measured


# ---- common randomness -----------------------------------------------------------------------------------------------
def noise_samples(n):
    """noise.py:17-54 in CPython floats, rounded to float32 as a float32 tensor holds them."""
    seed, a, m = 18101995, 16807, 2147483647
    out = np.empty(n, np.float32)
    for i in range(n):
        seed = (a * seed) % m
        u1 = seed / m
        seed = (a * seed) % m
        u2 = seed / m
        out[i] = math.sqrt(-2.0 * math.log(u1)) * math.cos(2.0 * 3.14159265359 * u2)
    return out


def _noise_chain(samples, level_sizes, dtype):
    import torch
    import torch.nn.functional as F

    grids, pos = [], 0
    for h, w in level_sizes:  # finest first
        grids.append(torch.from_numpy(samples[pos:pos + h * w].reshape(1, 1, h, w)).to(dtype))
        pos += h * w
    x = grids[-1]
    for target in reversed(grids[:-1]):
        x = F.interpolate(x, scale_factor=2, mode="bicubic", align_corners=False)[:, :, :target.shape[2], :target.shape[3]]
        x = torch.cat((target, x), dim=1)
    return x[0].numpy()


def noise_chain(level_sizes, samples=None):
    """(float64 planes [levels][h][w] of fixed_upsampling(mode="bicubic") over the noise grids, bar, measured): the bar by the
    rule of the module docstring, its measured term torch's float32 chain against the float64 one."""
    import torch

    n = sum(h * w for h, w in level_sizes)
    samples = noise_samples(n) if samples is None else samples[:n]
    ref64 = _noise_chain(samples, level_sizes, torch.float64)
    measured = float(np.abs(_noise_chain(samples, level_sizes, torch.float32).astype(np.float64) - ref64).max())
    return ref64, 2.0 * measured + FLOOR_ULPS * 2.0 ** -23 * float(np.abs(samples).max()), measured


# ---- integer planes --------------------------------------------------------------------------------------------------
def planes(out, bitdepth, frame_data_type):
    """decode.py:191-206 and the writers, literally, in torch float32: [3][H][W] float -> three uint16 planes."""
    import torch
    import torch.nn.functional as F

    maxv = float((1 << bitdepth) - 1)
    x = torch.from_numpy(np.ascontiguousarray(out, dtype=np.float32))
    x = torch.round(maxv * x) / maxv
    parts = [x[0], x[1], x[2]]
    if frame_data_type == 1:
        uv = F.avg_pool2d(x[1:3][None], 2)[0]
        parts = [x[0], uv[0], uv[1]]
    res = []
    for p in parts:
        p = torch.clamp(p, 0.0, 1.0)
        p = torch.round(p * maxv) / maxv
        res.append(torch.round(p * maxv).numpy().astype(np.uint16))
    return res
