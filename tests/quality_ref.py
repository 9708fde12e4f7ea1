"""numpy restatement of the quality meter's definitions (include/ccd.h, "quality of decoded frames") and the seeded
pictures the tests score.

PSNR: sse[p] = sum (dec - src)^2 as an exact integer; mse = sum_p sse[p] / (sum_p n[p] maxv^2); psnr = -10 log10(mse).
MS-SSIM (Wang, Simoncelli, Bovik 2003) per plane on x = sample / maxv: 5 scales, weights WEIGHTS, 11-tap Gaussian window
(sigma 1.5, normalised) applied separably and "valid", C1 = 0.01^2, C2 = 0.03^2, 2 x 2 mean with stride 2 between scales with a
trailing odd row / column dropped, ms_ssim = prod_{j<4} max(CS[j], 0)^w_j * max(SSIM[4], 0)^w_4.  A plane needs
floor(min(h, w) / 16) >= 11.

`dtype` selects the arithmetic of the maps and means (float64: the reference the device is held to; float32: the same
definition in single precision, whose distance from float64 is the floor the test's bound is derived from).  The final
product is always float64 from the ten means.

    python tests/quality_ref.py        prints that float32 floor over MS_CASES (the constants in tests/test_quality.py)
"""
import math

import numpy as np

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
N_SCALES = 5
WIN = 11
C1, C2 = 0.01 ** 2, 0.03 ** 2


def window(dtype=np.float64):
    g = np.exp(-((np.arange(WIN, dtype=np.float64) - 5.0) ** 2) / (2.0 * 1.5 ** 2))
    return (g / g.sum()).astype(dtype)


def sse(dec, src) -> int:
    d = dec.astype(np.int64) - src.astype(np.int64)
    return int((d * d).sum(dtype=np.int64))


def psnr(sse_list, n_list, bitdepth: int) -> float:
    maxv = float(2 ** bitdepth - 1)
    mse = float(sum(sse_list)) / (float(sum(n_list)) * maxv * maxv)
    return math.inf if mse == 0.0 else -10.0 * math.log10(mse)


def enough_for_ms_ssim(h: int, w: int) -> bool:
    return min(h, w) // 16 >= WIN


def _filter_valid(a, g):
    h, w = a.shape
    t = g[0] * a[:, 0:w - WIN + 1]
    for k in range(1, WIN):
        t = t + g[k] * a[:, k:k + w - WIN + 1]
    o = g[0] * t[0:h - WIN + 1]
    for k in range(1, WIN):
        o = o + g[k] * t[k:k + h - WIN + 1]
    return o


def scale_means(x, y, dtype=np.float64):
    """(mean of cs, mean of ssim) over the valid window positions of one scale; x, y already in [0, 1]."""
    g = window(dtype)
    c1, c2 = dtype(C1), dtype(C2)
    mx, my = _filter_valid(x, g), _filter_valid(y, g)
    sxx = _filter_valid(x * x, g) - mx * mx
    syy = _filter_valid(y * y, g) - my * my
    sxy = _filter_valid(x * y, g) - mx * my
    cs = (dtype(2) * sxy + c2) / (sxx + syy + c2)
    ss = (dtype(2) * mx * my + c1) / (mx * mx + my * my + c1) * cs
    return float(cs.mean(dtype=dtype)), float(ss.mean(dtype=dtype))


def pool2(a):
    h, w = a.shape
    a = a[:h // 2 * 2, :w // 2 * 2]
    return (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]) * a.dtype.type(0.25)


def combine(cs, ssim) -> float:
    v = 1.0
    for j in range(N_SCALES):
        t = cs[j] if j + 1 < N_SCALES else ssim[j]
        v *= max(float(t), 0.0) ** WEIGHTS[j]
    return v


def ms_ssim_plane(dec, src, bitdepth: int, dtype=np.float64):
    """{"n_scales", "cs", "ssim", "ms_ssim"} of one plane; n_scales = 0 and ms_ssim = NaN when it is too small."""
    h, w = dec.shape
    if not enough_for_ms_ssim(h, w):
        return {"n_scales": 0, "cs": [], "ssim": [], "ms_ssim": math.nan}
    maxv = dtype(2 ** bitdepth - 1)
    x, y = src.astype(dtype) / maxv, dec.astype(dtype) / maxv
    cs, ss = [], []
    for j in range(N_SCALES):
        c, s = scale_means(x, y, dtype)
        cs.append(c)
        ss.append(s)
        if j + 1 < N_SCALES:
            x, y = pool2(x), pool2(y)
    return {"n_scales": N_SCALES, "cs": cs, "ssim": ss, "ms_ssim": combine(cs, ss)}


def frame_ms_ssim(per_plane, frame_data_type: str) -> float:
    """rgb / yuv444: mean over the three planes; yuv420: the luma plane."""
    return per_plane[0] if frame_data_type == "yuv420" else sum(per_plane) / 3.0


def ms_ssim_db(v: float) -> float:
    if math.isnan(v):
        return math.nan
    return math.inf if v >= 1.0 else -10.0 * math.log10(1.0 - v)


# ---- the pictures the tests score: everything comes from a seed ----------------------------------------------------------
def textured(seed: int, h: int, w: int, bitdepth: int):
    """A smooth picture with edges and fine texture, on the integer grid of `bitdepth`."""
    rng = np.random.default_rng(seed)
    maxv = 2 ** bitdepth - 1
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    a, b, c = rng.uniform(0.0, 6.28, 3)
    v = 0.5 + 0.22 * np.sin(xx / 17.0 + a) * np.cos(yy / 23.0 + b) + 0.15 * np.sin((xx + 2.0 * yy) / 61.0 + c)
    v += 0.12 * (((xx // 48) + (yy // 40)) % 2) + 0.03 * rng.standard_normal((h, w))
    dt = np.uint8 if bitdepth == 8 else np.uint16
    return np.clip(np.rint(v * maxv), 0, maxv).astype(dt)


def with_noise(src, seed: int, bitdepth: int, sigma: float):
    """src plus Gaussian noise of standard deviation sigma x maxv, clipped to the sample range."""
    rng = np.random.default_rng(seed)
    maxv = 2 ** bitdepth - 1
    v = src.astype(np.float64) + np.rint(rng.standard_normal(src.shape) * sigma * maxv)
    return np.clip(v, 0, maxv).astype(src.dtype)


def flat_pair(seed: int, h: int, w: int, bitdepth: int):
    """The cancellation case: a flat mid-grey source, and the same with about one sample in 97 moved by +-1."""
    rng = np.random.default_rng(seed)
    dt = np.uint8 if bitdepth == 8 else np.uint16
    src = np.full((h, w), (2 ** bitdepth - 1) // 2, dtype=dt)
    hit = rng.random((h, w)) < 1.0 / 97.0
    step = np.where(rng.random((h, w)) < 0.5, -1, 1)
    return (src.astype(np.int64) + hit * step).astype(dt), src


LIGHT, HEAVY = 0.01, 0.15  # noise levels (standard deviation / maxv)
# (name, h, w, bit depth, planes): the shapes the MS-SSIM comparison runs at; each is scored with light noise, heavy noise
# and as the flat picture with isolated +-1 samples
MS_SHAPES = [("rgb512x768", 512, 768, 8, 3), ("b10_540x960", 540, 960, 10, 1), ("b16_177x200", 177, 200, 16, 1),
             ("b8_1365x2048", 1365, 2048, 8, 1), ("b10_2160x3840", 2160, 3840, 10, 1)]
MS_KINDS = ("light", "heavy", "flat")
MS_CASES = [(name, kind) for name, *_ in MS_SHAPES for kind in MS_KINDS]


def ms_case(name: str, kind: str):
    """-> (decoded planes, source planes, bit depth) of one case."""
    idx = [s[0] for s in MS_SHAPES].index(name)
    _, h, w, bd, n_planes = MS_SHAPES[idx]
    dec, src = [], []
    for p in range(n_planes):
        seed = 1000 * (idx + 1) + 10 * p + MS_KINDS.index(kind)
        if kind == "flat":
            d, s = flat_pair(seed, h, w, bd)
        else:
            s = textured(seed, h, w, bd)
            d = with_noise(s, seed + 500, bd, LIGHT if kind == "light" else HEAVY)
        dec.append(d)
        src.append(s)
    return dec, src, bd


def float32_floor():
    """Largest distance between the float32 and the float64 evaluation over MS_CASES: (per-scale means, ms_ssim)."""
    worst_mean, worst_ms = 0.0, 0.0
    for name, kind in MS_CASES:
        dec, src, bd = ms_case(name, kind)
        for d, s in zip(dec, src):
            lo, hi = ms_ssim_plane(d, s, bd, np.float32), ms_ssim_plane(d, s, bd, np.float64)
            dm = max(abs(a - b) for a, b in zip(lo["cs"] + lo["ssim"], hi["cs"] + hi["ssim"]))
            ds = abs(lo["ms_ssim"] - hi["ms_ssim"])
            print(f"{name:16s} {kind:6s} means {dm:.3e}  ms_ssim {ds:.3e}  (ms_ssim = {hi['ms_ssim']:.9f})")
            worst_mean, worst_ms = max(worst_mean, dm), max(worst_ms, ds)
    return worst_mean, worst_ms


if __name__ == "__main__":
    m, s = float32_floor()
    print(f"F32_FLOOR_MEANS = {m:.3e}\nF32_FLOOR_MS_SSIM = {s:.3e}")
