"""An independent float64 restatement of P / B frame reconstruction (decode.py:156-206), for the tests of
tests/test_inter_reconstruct.py.  Written from what the reference does - not from the oracle's or the kernel's float32
formulas - so that a mistake those two share still shows:

  reference planes  integer planes -> q / (2^bd - 1); 4:2:0 chroma repeated 2 x 2 (nearest x2, yuv.py:303-316)
  global flow       integer translation, border replicate (globalmotion.py:151-160)
  warp 2 / 4 taps   F.grid_sample(bilinear | bicubic, padding_mode="border", align_corners=True) on
                    grid = linspace(-1, 1, n) + flow / ((n - 1) / 2)   (warp.py:92-116, 325-343), CPU, float64
  warp 6..16 taps   coef_j = cos(pi d / N) sinc(d), d = frac(flow) - (j - N/2 + 1), taps at floor(flow) + j - N/2 + 1
                    (warp.py:226-243, 294-397), indices in int64 clamped to the picture: any flow beyond the picture
                    reads the border
  blend             alpha, beta = clip(residue[3 | 4] + 0.5, 0, 1); pred = beta w0 + (1 - beta) w1; x = alpha pred + residue
  quantise          round(x (2^bd - 1)), clipped; 4:2:0 chroma: every sample rounded to the bit-depth grid, then the
                    2 x 2 mean, clipped, rounded (decode.py:191-206)

Flows must be finite: a non-finite flow makes NaN here."""
import numpy as np


def planes_to_444(planes, bitdepth: int, frame_data_type: int) -> np.ndarray:
    maxv = float(2 ** bitdepth - 1)
    y = np.asarray(planes[0], dtype=np.float64)
    out = [y / maxv]
    for p in planes[1:]:
        p = np.asarray(p, dtype=np.float64)
        if frame_data_type == 1:
            p = np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
        out.append(p / maxv)
    return np.stack(out)


def global_shift(ref: np.ndarray, gx: int, gy: int) -> np.ndarray:
    """ref[:, clip(y + gy), clip(x + gx)]"""
    _, h, w = ref.shape
    ys = np.clip(np.arange(h, dtype=np.int64) + gy, 0, h - 1)
    xs = np.clip(np.arange(w, dtype=np.int64) + gx, 0, w - 1)
    return ref[:, ys][:, :, xs]


def warp_grid_sample(ref: np.ndarray, fx: np.ndarray, fy: np.ndarray, n_taps: int) -> np.ndarray:
    import torch
    import torch.nn.functional as F

    _, h, w = ref.shape
    gx = torch.linspace(-1.0, 1.0, w, dtype=torch.float64)[None, :] + torch.from_numpy(np.asarray(fx, np.float64)) / ((w - 1) / 2)
    gy = torch.linspace(-1.0, 1.0, h, dtype=torch.float64)[:, None] + torch.from_numpy(np.asarray(fy, np.float64)) / ((h - 1) / 2)
    grid = torch.stack([gx, gy], dim=-1)[None]
    out = F.grid_sample(torch.from_numpy(ref)[None], grid, mode="bilinear" if n_taps == 2 else "bicubic", padding_mode="border",
                        align_corners=True)
    return out[0].numpy()


def sinc_coefficients(frac: np.ndarray, n_taps: int) -> np.ndarray:
    """[..., n_taps]: cos(pi d / N) sinc(d), d = frac - (j - N/2 + 1)"""
    rel = np.arange(n_taps, dtype=np.float64) - n_taps // 2 + 1
    d = frac[..., None] - rel
    return np.cos(np.pi * d / n_taps) * np.sinc(d)


def warp_sinc(ref: np.ndarray, fx: np.ndarray, fy: np.ndarray, n_taps: int, gx: int, gy: int) -> np.ndarray:
    """The N-tap sinc warp of the globally shifted reference; `ref` unshifted (both clamps on the integer index)."""
    _, h, w = ref.shape
    fx = np.asarray(fx, np.float64)
    fy = np.asarray(fy, np.float64)
    rx, ry = np.floor(fx), np.floor(fy)
    cx, cy = sinc_coefficients(fx - rx, n_taps), sinc_coefficients(fy - ry, n_taps)
    rel = np.arange(n_taps, dtype=np.int64) - n_taps // 2 + 1
    xs = np.arange(w, dtype=np.int64)[None, :, None] + rx.astype(np.int64)[..., None] + rel      # [h, w, N]
    ys = np.arange(h, dtype=np.int64)[:, None, None] + ry.astype(np.int64)[..., None] + rel
    xs = np.clip(np.clip(xs, 0, w - 1) + gx, 0, w - 1)
    ys = np.clip(np.clip(ys, 0, h - 1) + gy, 0, h - 1)
    out = np.empty_like(ref)
    for c in range(ref.shape[0]):
        taps = ref[c][ys[:, :, :, None], xs[:, :, None, :]]                                      # [h, w, N (y), N (x)]
        out[c] = np.einsum("hwij,hwi,hwj->hw", taps, cy, cx)
    return out


def warp(ref: np.ndarray, fx, fy, n_taps: int, gx: int, gy: int) -> np.ndarray:
    if n_taps in (2, 4):
        return warp_grid_sample(global_shift(ref, gx, gy), fx, fy, n_taps)
    return warp_sinc(ref, fx, fy, n_taps, gx, gy)


def quantise(img: np.ndarray, bitdepth: int, frame_data_type: int):
    maxv = float(2 ** bitdepth - 1)
    if frame_data_type != 1:
        return [np.clip(np.rint(p * maxv), 0, maxv).astype(np.int64) for p in img]
    out = [np.clip(np.rint(img[0] * maxv), 0, maxv).astype(np.int64)]
    h, w = img.shape[1:]
    for p in img[1:]:
        q = np.rint(p[: h // 2 * 2, : w // 2 * 2] * maxv)
        m = (q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2]) / 4.0
        out.append(np.clip(np.rint(m), 0, maxv).astype(np.int64))
    return out


def inter_reconstruct(frame_type: int, residue: np.ndarray, motion: np.ndarray, ref0, ref1, global_flow, n_taps: int, bitdepth: int,
                      frame_data_type: int):
    """Integer planes (int64) of one P (1) / B (2) frame; ref0 / ref1 = integer planes as stored (half-size chroma for 4:2:0)."""
    res = np.asarray(residue, np.float64)
    mot = np.asarray(motion, np.float64)
    gf = list(global_flow) + [0, 0, 0, 0]
    w0 = warp(planes_to_444(ref0, bitdepth, frame_data_type), mot[0], mot[1], n_taps, gf[0], gf[1])
    alpha = np.clip(res[3] + 0.5, 0.0, 1.0)
    if frame_type == 2:
        w1 = warp(planes_to_444(ref1, bitdepth, frame_data_type), mot[2], mot[3], n_taps, gf[2], gf[3])
        beta = np.clip(res[4] + 0.5, 0.0, 1.0)
        pred = beta * w0 + (1.0 - beta) * w1
    else:
        pred = w0
    return quantise(alpha * pred + res[:3], bitdepth, frame_data_type)
