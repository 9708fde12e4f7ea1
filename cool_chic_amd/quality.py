"""PSNR and MS-SSIM of decoded frames against their source, scored on the MI355X (C ABI: ccd_quality_* in
include/ccd.h, kernels in csrc/ccd_quality.hip).

The reference scores a picture right after its own decode (cc_encode.py:461-505: decode_video, then PSNR and rate into
*-results_decoder.tsv).  Here the decoded integer planes already sit in HBM, so they are compared there: the squared error
comes back as exact integers, MS-SSIM as ten spatial means per plane, and only those cross PCIe.

PSNR is the reference's (training/metrics/mse.py:14-21, loss.py:88-118): -10 log10(sum of squared errors / (samples x
maxv^2)) over all planes of the frame, which for 4:2:0 is its plane-size-weighted MSE.  The reference has no MS-SSIM; the
definition used here (Wang, Simoncelli, Bovik 2003; valid 11-tap Gaussian windows, 2 x 2 mean between scales without
padding) is stated in include/ccd.h and restated in numpy in tests/quality_ref.py."""
import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._handle import _Handle
from ._lib import QualityItem, QualityResult, check, lib
from .batch import FRAME_DATA_TYPES
from .io import FrameData

PSNR, MS_SSIM = 1, 2  # CCD_QUALITY_PSNR, CCD_QUALITY_MS_SSIM
RESULT_COLUMNS = ("display_index", "frame_type", "n_pixels", "n_bytes", "rate_bpp", "psnr_db", "psnr_0", "psnr_1", "psnr_2",
                  "ms_ssim", "ms_ssim_db")


@dataclass
class FrameQuality:
    """What the device measured for one frame (sse, n, n_scales, cs, ssim per plane) and what follows from it on the host."""

    bitdepth: int
    frame_data_type: str
    sse: Tuple[int, int, int]
    n: Tuple[int, int, int]
    n_scales: Tuple[int, int, int]
    cs: Tuple[Tuple[float, ...], ...]      # [plane][scale] spatial means
    ssim: Tuple[Tuple[float, ...], ...]
    psnr_db: float = float("nan")
    psnr_planes: Tuple[float, float, float] = (float("nan"),) * 3
    ms_ssim_planes: Tuple[float, float, float] = (float("nan"),) * 3
    ms_ssim: float = float("nan")          # rgb / yuv444: mean over the three planes; yuv420: the luma plane
    ms_ssim_db: float = float("nan")

    def __post_init__(self):
        r = self.as_result()
        L = lib()
        self.psnr_db = L.ccd_quality_psnr(C.byref(r), self.bitdepth, -1)
        self.psnr_planes = tuple(L.ccd_quality_psnr(C.byref(r), self.bitdepth, p) for p in range(3))
        self.ms_ssim_planes = tuple(L.ccd_quality_ms_ssim(C.byref(r), p) for p in range(3))
        self.ms_ssim = self.ms_ssim_planes[0] if self.frame_data_type == "yuv420" else sum(self.ms_ssim_planes) / 3.0
        if math.isnan(self.ms_ssim):
            self.ms_ssim_db = float("nan")
        else:
            self.ms_ssim_db = float("inf") if self.ms_ssim >= 1.0 else -10.0 * math.log10(1.0 - self.ms_ssim)

    def as_result(self) -> QualityResult:
        r = QualityResult()
        for p in range(3):
            r.sse[p], r.n[p], r.n_scales[p] = int(self.sse[p]), int(self.n[p]), int(self.n_scales[p])
            for j in range(5):
                r.cs[p][j] = self.cs[p][j] if j < len(self.cs[p]) else 0.0
                r.ssim[p][j] = self.ssim[p][j] if j < len(self.ssim[p]) else 0.0
        return r

    @classmethod
    def from_result(cls, r: QualityResult, bitdepth: int, frame_data_type: str) -> "FrameQuality":
        return cls(bitdepth, frame_data_type, tuple(int(v) for v in r.sse), tuple(int(v) for v in r.n),
                   tuple(int(v) for v in r.n_scales), tuple(tuple(r.cs[p]) for p in range(3)),
                   tuple(tuple(r.ssim[p]) for p in range(3)))


def _make_items(geometries) -> "C.Array":
    """geometries: per frame (dec addresses[3], src addresses[3], h, w, ch, cw, bitdepth)."""
    arr = (QualityItem * max(len(geometries), 1))()
    for a, (dec, src, h, w, ch, cw, bd) in zip(arr, geometries):
        for p in range(3):
            a.dec[p], a.src[p] = dec[p], src[p]
        a.h, a.w, a.ch, a.cw, a.bitdepth = int(h), int(w), int(ch), int(cw), int(bd)
    return arr


def scratch_bytes(geometries, what: int = PSNR | MS_SSIM) -> int:
    """Bytes of device scratch a scoring of these frames takes (host only; raises on what the library refuses)."""
    return check(lib().ccd_quality_scratch_bytes(_make_items(geometries), len(geometries), int(what)), "ccd_quality_scratch_bytes")


def _frame_planes(fd: FrameData, device: torch.device) -> List[torch.Tensor]:
    from .bitstream.intercoding import _integer_planes

    return _integer_planes(fd, device)


def scored_frame_type(fd: FrameData) -> int:
    """The index of the frame's sample format in FRAME_DATA_TYPES; a format that has no planes to score raises."""
    if fd.frame_data_type not in ("rgb", "yuv420", "yuv444"):
        raise ValueError(f"cannot score a {fd.frame_data_type} frame")
    return FRAME_DATA_TYPES.index(fd.frame_data_type)


class QualityMeter(_Handle):
    """One meter = one handle; a scoring is enqueued on the current stream of its device and waited for."""

    _destroy = "ccd_quality_destroy"

    def __init__(self, device: int = 0):
        self._open("ccd_quality_create", device)

    def score_planes_async(self, decoded: Sequence[Sequence[torch.Tensor]], sources: Sequence[Sequence[torch.Tensor]],
                           bitdepths: Sequence[int], ms_ssim: bool = True, stream: Optional[int] = None) -> None:
        """decoded[i], sources[i]: the three integer planes of frame i as contiguous CUDA tensors (uint8 at 8 bits, uint16
        above), read in place.  Only enqueues; the tensors must stay alive until finish()."""
        geo = []
        for dec, src, bd in zip(decoded, sources, bitdepths):
            if len(dec) != 3 or len(src) != 3:
                raise ValueError("a frame has three planes")
            dt = torch.uint8 if bd == 8 else torch.uint16
            for d, s in zip(dec, src):
                if d.shape != s.shape or d.dim() != 2:
                    raise ValueError(f"decoded plane is {tuple(d.shape)}, source plane {tuple(s.shape)}")
                for t in (d, s):
                    if not t.is_cuda or (t.device.index or 0) != self.device or t.dtype != dt or not t.is_contiguous():
                        raise ValueError(f"planes must be contiguous {dt} tensors on cuda:{self.device}")
            if dec[1].shape != dec[2].shape:
                raise ValueError("the two chroma planes differ in size")
            geo.append(([d.data_ptr() for d in dec], [s.data_ptr() for s in src], dec[0].shape[0], dec[0].shape[1],
                        dec[1].shape[0], dec[1].shape[1], bd))
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        self._stream, self._n = stream, len(geo)
        check(lib().ccd_quality_score_batch(self._h, _make_items(geo), len(geo), PSNR | (MS_SSIM if ms_ssim else 0),
                                            C.c_void_p(stream or None)), "ccd_quality_score_batch")

    def finish(self) -> List[QualityResult]:
        res = (QualityResult * self._n)()
        check(lib().ccd_quality_finish_batch(self._h, C.c_void_p(self._stream or None), res, self._n), "ccd_quality_finish_batch")
        return list(res)

    def score_planes(self, decoded, sources, bitdepths, frame_data_types=None, ms_ssim: bool = True) -> List[FrameQuality]:
        """Integer CUDA planes in, one FrameQuality per frame out (one set of launches for the whole list)."""
        if len(decoded) == 0:
            return []
        fdts = frame_data_types or ["rgb"] * len(decoded)
        self.score_planes_async(decoded, sources, bitdepths, ms_ssim)
        return [FrameQuality.from_result(r, bd, fdt) for r, bd, fdt in zip(self.finish(), bitdepths, fdts)]

    def score(self, frames: Sequence[FrameData], sources: Sequence[FrameData], ms_ssim: bool = True) -> List[FrameQuality]:
        """Decoded frames against their sources.  Data already on the GPU stays there; host data is uploaded once."""
        if len(frames) != len(sources):
            raise ValueError(f"{len(frames)} decoded frames, {len(sources)} sources")
        dev = torch.device(f"cuda:{self.device}")
        for f, s in zip(frames, sources):
            _check_like(s.bitdepth, s.frame_data_type, s.img_size, f)
        dec = [_frame_planes(f, dev) for f in frames]
        src = [_frame_planes(s, dev) for s in sources]
        return self.score_planes(dec, src, [f.bitdepth for f in frames], [f.frame_data_type for f in frames], ms_ssim)


# ---- sources ---------------------------------------------------------------------------------------------------------
def _check_like(bitdepth: int, frame_data_type: str, img_size, like: FrameData) -> None:
    if tuple(img_size) != tuple(like.img_size):
        raise ValueError(f"source is {img_size[0]}x{img_size[1]}, the decoded frame {like.img_size[0]}x{like.img_size[1]}")
    if bitdepth != like.bitdepth or frame_data_type != like.frame_data_type:
        raise ValueError(f"source is {frame_data_type} {bitdepth}-bit, the decoded frame {like.frame_data_type} {like.bitdepth}-bit")


def _planes_to_frame_data(planes: List[np.ndarray], bitdepth: int, frame_data_type: str) -> FrameData:
    maxv = float(2 ** bitdepth - 1)
    f = [torch.from_numpy(np.ascontiguousarray(p).astype(np.float32)).div(maxv)[None, None] for p in planes]
    if frame_data_type == "yuv420":
        return FrameData(bitdepth, frame_data_type, {"y": f[0], "u": f[1], "v": f[2]})
    return FrameData(bitdepth, frame_data_type, torch.cat(f, dim=1))


def _read_ppm(path: str):
    """Binary P6 (io/format/ppm.py:161-203 writes it): "P6 W H MAX" separated by white space, '#' comments, then one white
    space byte and interleaved RGB, big-endian above 8 bits."""
    with open(path, "rb") as f:
        raw = f.read()
    tokens, at = [], 0
    while len(tokens) < 4:
        while at < len(raw) and raw[at:at + 1].isspace():
            at += 1
        if raw[at:at + 1] == b"#":
            while at < len(raw) and raw[at:at + 1] != b"\n":
                at += 1
            continue
        start = at
        while at < len(raw) and not raw[at:at + 1].isspace():
            at += 1
        if start == at:
            raise ValueError(f"{path}: truncated PPM header")
        tokens.append(raw[start:at])
    at += 1  # the single white space after MAX
    if tokens[0] != b"P6":
        raise ValueError(f"{path}: not a binary PPM (P6)")
    w, h, maxv = int(tokens[1]), int(tokens[2]), int(tokens[3])
    if maxv < 1 or maxv > 65535 or (maxv + 1) & maxv:
        raise ValueError(f"{path}: maximum value {maxv} is not 2^bitdepth - 1")
    dt = np.dtype(">u2") if maxv > 255 else np.dtype(np.uint8)
    if len(raw) - at < h * w * 3 * dt.itemsize:
        raise ValueError(f"{path}: truncated PPM data")
    img = np.frombuffer(raw, dtype=dt, count=h * w * 3, offset=at).reshape(h, w, 3)
    return [img[:, :, c].astype(np.uint16) for c in range(3)], maxv.bit_length()


def read_source(path: str, like: FrameData, frame_index: int = 0) -> FrameData:
    """The source picture of a decoded frame, as a FrameData on the host with `like`'s size, format and bit depth.
    .png: 8-bit RGB (PIL); .ppm: binary P6, 8 to 16 bits; .yuv: planar, frame `frame_index` of the file, geometry, chroma
    format and bit depth taken from `like` (one byte per sample at 8 bits, two little-endian bytes above).
    A source of another size or format than `like` is a ValueError."""
    ext = os.path.splitext(path)[1].lower()
    h, w = like.img_size
    if ext == ".png":
        from PIL import Image

        with Image.open(path) as im:
            img = np.asarray(im.convert("RGB"))
        _check_like(8, "rgb", img.shape[:2], like)
        return _planes_to_frame_data([img[:, :, c] for c in range(3)], 8, "rgb")
    if ext == ".ppm":
        planes, bitdepth = _read_ppm(path)
        _check_like(max(bitdepth, 8), "rgb", planes[0].shape, like)
        return _planes_to_frame_data(planes, like.bitdepth, "rgb")
    if ext == ".yuv":
        if like.frame_data_type not in ("yuv420", "yuv444"):
            raise ValueError(f"a .yuv source cannot be compared with a {like.frame_data_type} frame")
        ch, cw = (h // 2, w // 2) if like.frame_data_type == "yuv420" else (h, w)
        dt = np.dtype(np.uint8) if like.bitdepth == 8 else np.dtype("<u2")
        n_frame = (h * w + 2 * ch * cw) * dt.itemsize
        size = os.path.getsize(path)
        if size % n_frame:
            raise ValueError(f"{path}: {size} bytes is not a whole number of {w}x{h} {like.frame_data_type} "
                             f"{like.bitdepth}-bit frames ({n_frame} bytes each)")
        if frame_index < 0 or (frame_index + 1) * n_frame > size:
            raise ValueError(f"{path}: no frame {frame_index} ({size // n_frame} frames)")
        with open(path, "rb") as f:
            f.seek(frame_index * n_frame)
            raw = np.frombuffer(f.read(n_frame), dtype=dt)
        if int(raw.max(initial=0)) > 2 ** like.bitdepth - 1:
            raise ValueError(f"{path}: a sample exceeds {like.bitdepth} bits")
        planes = [raw[:h * w].reshape(h, w), raw[h * w:h * w + ch * cw].reshape(ch, cw), raw[h * w + ch * cw:].reshape(ch, cw)]
        return _planes_to_frame_data(planes, like.bitdepth, like.frame_data_type)
    raise ValueError(f"expected a .png, .ppm or .yuv source, found {path}")


# ---- results file ----------------------------------------------------------------------------------------------------
def _mean(values) -> float:
    values = list(values)
    return sum(values) / len(values) if values else float("nan")


def write_results(path: str, rows, n_bytes_video_header: int = 0) -> None:
    """Tab-separated results, the counterpart of the reference's *-results_decoder.tsv: one row per frame in display order
    and a last row `all` with the total rate and the mean of the per-frame values (the JVET convention).
    rows: (display_index, frame_type, n_pixels, n_bytes, FrameQuality) per frame; n_bytes is what the frame took in the
    stream, the video header is counted in the `all` row only."""
    rows = sorted(rows, key=lambda r: r[0])

    def line(first, frame_type, n_pixels, n_bytes, values):
        rate = 8.0 * n_bytes / n_pixels if n_pixels else float("nan")
        return "\t".join([str(first), frame_type, str(n_pixels), str(n_bytes), repr(float(rate))] + [repr(float(v)) for v in values])

    per_frame = [(q.psnr_db, q.psnr_planes[0], q.psnr_planes[1], q.psnr_planes[2], q.ms_ssim, q.ms_ssim_db) for *_, q in rows]
    with open(path, "w") as f:
        f.write("\t".join(RESULT_COLUMNS) + "\n")
        for (di, ft, n_px, n_b, _), values in zip(rows, per_frame):
            f.write(line(di, ft, n_px, n_b, values) + "\n")
        f.write(line("all", "-", sum(r[2] for r in rows), sum(r[3] for r in rows) + int(n_bytes_video_header),
                     [_mean(v[k] for v in per_frame) for k in range(6)]) + "\n")
