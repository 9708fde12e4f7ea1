"""The quality meter (ccd_quality_*, cool_chic_amd/quality.py): PSNR and MS-SSIM of decoded planes against their source.

The squared error is exact: no tolerance.  MS-SSIM is compared with the float64 numpy restatement (tests/quality_ref.py).
Its bound comes from the definition itself, not from the kernel: the same restatement evaluated in float32 differs from
float64 by the floors below on this file's own inputs (measured on the CPU with `python tests/quality_ref.py`, which
prints every case and the two maxima per kind of picture), and the device is allowed twice that floor."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import quality_ref as ref
from conftest import GOLDEN, ROOT, load_golden, reference_planes

# `python tests/quality_ref.py`: largest |float32 - float64| of the restatement over MS_CASES, textured pictures (light and
# heavy noise) and the flat picture with isolated +-1 samples (where float32 loses the variance subtraction)
F32_FLOOR_MEANS_TEXTURED = 1.059e-06
F32_FLOOR_MS_SSIM_TEXTURED = 1.828e-07
F32_FLOOR_MEANS_FLAT = 2.051e-05
F32_FLOOR_MS_SSIM_FLAT = 1.104e-05

ERR_ARG = -7


def _lib():
    from cool_chic_amd._lib import lib

    return lib()


def _items(specs):
    """specs: (h, w, ch, cw, bitdepth) with made-up, never dereferenced plane addresses."""
    from cool_chic_amd._lib import QualityItem

    arr = (QualityItem * len(specs))()
    for a, (h, w, ch, cw, bd) in zip(arr, specs):
        for p in range(3):
            a.dec[p], a.src[p] = 4096 * (p + 1), 4096 * (p + 4)
        a.h, a.w, a.ch, a.cw, a.bitdepth = h, w, ch, cw, bd
    return arr


# ---- CPU: validation without a device -----------------------------------------------------------------------------------
def test_scratch_bytes_validates_and_grows():
    L = _lib()
    good = (512, 768, 512, 768, 8)
    one = L.ccd_quality_scratch_bytes(_items([good]), 1, 3)
    two = L.ccd_quality_scratch_bytes(_items([good, good]), 2, 3)
    assert 0 < one < two
    assert 0 < L.ccd_quality_scratch_bytes(_items([good]), 1, 1) < one  # PSNR alone needs no pooled pictures
    assert L.ccd_quality_scratch_bytes(_items([(1, 1, 1, 1, 16)]), 1, 3) > 0
    assert L.ccd_quality_scratch_bytes(_items([(16383, 16383, 8191, 8191, 12)]), 1, 3) > 0


@pytest.mark.parametrize("spec", [(0, 768, 1, 1, 8), (512, 0, 1, 1, 8), (512, 768, 0, 384, 8), (512, 768, 256, 0, 8),
                                  (16384, 768, 1, 1, 8), (512, 16384, 1, 1, 8), (512, 768, 16384, 1, 8), (512, 768, 1, 16384, 8),
                                  (512, 768, 512, 768, 7), (512, 768, 512, 768, 17), (-5, 768, 1, 1, 8)])
def test_scratch_bytes_rejects_bad_item(spec):
    L = _lib()
    good = (512, 768, 512, 768, 8)
    assert L.ccd_quality_scratch_bytes(_items([spec]), 1, 3) == ERR_ARG
    assert L.ccd_quality_scratch_bytes(_items([good, spec]), 2, 3) == ERR_ARG  # not only the first item is looked at


def test_bad_arguments_without_device():
    from cool_chic_amd._lib import QualityResult

    L = _lib()
    good = _items([(512, 768, 512, 768, 8)])
    assert L.ccd_quality_scratch_bytes(None, 1, 3) == ERR_ARG
    assert L.ccd_quality_scratch_bytes(good, -1, 3) == ERR_ARG
    assert L.ccd_quality_scratch_bytes(good, 0, 3) == ERR_ARG
    for what in (0, 4, 7, -1):
        assert L.ccd_quality_scratch_bytes(good, 1, what) == ERR_ARG
    for plane, which in ((1, "dec"), (2, "src")):
        bad = _items([(512, 768, 512, 768, 8)])
        getattr(bad[0], which)[plane] = None
        assert L.ccd_quality_scratch_bytes(bad, 1, 3) == ERR_ARG
    res = (QualityResult * 1)()
    assert L.ccd_quality_score_batch(None, good, 1, 3, None) == ERR_ARG
    assert L.ccd_quality_finish_batch(None, None, res, 1) == ERR_ARG
    assert L.ccd_quality_create(0, None) == ERR_ARG
    L.ccd_quality_destroy(None)  # a no-op


def _result(sse, n, n_scales=(0, 0, 0), cs=None, ssim=None):
    from cool_chic_amd._lib import QualityResult

    r = QualityResult()
    for p in range(3):
        r.sse[p], r.n[p], r.n_scales[p] = sse[p], n[p], n_scales[p]
        for j in range(5):
            r.cs[p][j] = cs[p][j] if cs else 0.0
            r.ssim[p][j] = ssim[p][j] if ssim else 0.0
    return r


def test_psnr_and_ms_ssim_from_hand_made_results():
    L = _lib()
    ones = [[1.0] * 5] * 3
    same = _result((0, 0, 0), (16, 16, 16), (5, 5, 5), ones, ones)
    assert L.ccd_quality_psnr(C.byref(same), 8, -1) == math.inf
    assert all(L.ccd_quality_psnr(C.byref(same), 8, p) == math.inf for p in range(3))
    assert all(L.ccd_quality_ms_ssim(C.byref(same), p) == 1.0 for p in range(3))
    # one sample off by one in an 8-bit 3 x 4 x 4 frame
    off = _result((0, 1, 0), (16, 16, 16))
    assert L.ccd_quality_psnr(C.byref(off), 8, -1) == pytest.approx(10.0 * math.log10(48 * 255 ** 2), rel=1e-15)
    assert L.ccd_quality_psnr(C.byref(off), 8, 1) == pytest.approx(10.0 * math.log10(16 * 255 ** 2), rel=1e-15)
    assert L.ccd_quality_psnr(C.byref(off), 8, 0) == math.inf
    # 4:2:0: total squared error over total samples (the plane-size-weighted MSE), 10-bit
    yuv = _result((5000, 300, 70), (64 * 48, 32 * 24, 32 * 24))
    want = -10.0 * math.log10((5000 + 300 + 70) / ((64 * 48 + 2 * 32 * 24) * 1023.0 ** 2))
    assert L.ccd_quality_psnr(C.byref(yuv), 10, -1) == pytest.approx(want, rel=1e-15)
    assert L.ccd_quality_psnr(C.byref(yuv), 10, -1) == pytest.approx(ref.psnr([5000, 300, 70], [3072, 768, 768], 10), rel=1e-15)
    # too small for MS-SSIM
    assert math.isnan(L.ccd_quality_ms_ssim(C.byref(yuv), 0))
    # the product of the ten means: CS of scales 0..3, SSIM of scale 4; negative means clamp to 0
    cs = [[0.9, 0.8, 0.95, 0.7, 0.1]] * 3
    ss = [[0.2, 0.3, 0.4, 0.5, 0.85]] * 3
    r = _result((1, 1, 1), (9, 9, 9), (5, 5, 5), cs, ss)
    want = 0.9 ** 0.0448 * 0.8 ** 0.2856 * 0.95 ** 0.3001 * 0.7 ** 0.2363 * 0.85 ** 0.1333
    assert L.ccd_quality_ms_ssim(C.byref(r), 2) == pytest.approx(want, rel=1e-14)
    assert L.ccd_quality_ms_ssim(C.byref(r), 2) == pytest.approx(ref.combine(cs[0], ss[0]), rel=1e-14)
    neg = _result((1, 1, 1), (9, 9, 9), (5, 5, 5), [[0.9, -0.2, 0.9, 0.9, 0.9]] * 3, ss)
    assert L.ccd_quality_ms_ssim(C.byref(neg), 0) == 0.0
    # bad selectors
    assert math.isnan(L.ccd_quality_psnr(None, 8, -1)) and math.isnan(L.ccd_quality_psnr(C.byref(off), 8, 3))
    assert math.isnan(L.ccd_quality_psnr(C.byref(off), 7, -1)) and math.isnan(L.ccd_quality_ms_ssim(C.byref(r), 3))


def test_frame_quality_per_frame_rules():
    from cool_chic_amd.quality import FrameQuality

    cs = ((0.9,) * 5, (0.8,) * 5, (0.7,) * 5)
    q444 = FrameQuality(8, "rgb", (4, 5, 6), (100, 100, 100), (5, 5, 5), cs, cs)
    per_plane = [ref.combine(c, c) for c in cs]
    assert q444.ms_ssim == pytest.approx(sum(per_plane) / 3.0, rel=1e-14)
    assert q444.ms_ssim_db == pytest.approx(-10.0 * math.log10(1.0 - q444.ms_ssim), rel=1e-14)
    q420 = FrameQuality(8, "yuv420", (4, 5, 6), (400, 100, 100), (5, 0, 0), cs, cs)
    assert q420.ms_ssim == pytest.approx(per_plane[0], rel=1e-14) and math.isnan(q420.ms_ssim_planes[1])
    assert q420.psnr_db == pytest.approx(ref.psnr([4, 5, 6], [400, 100, 100], 8), rel=1e-15)
    small = FrameQuality(8, "rgb", (0, 0, 0), (4, 4, 4), (0, 0, 0), ((),) * 3, ((),) * 3)
    assert small.psnr_db == math.inf and math.isnan(small.ms_ssim) and math.isnan(small.ms_ssim_db)


# ---- CPU: the numpy restatement against closed forms -----------------------------------------------------------------
def test_reference_closed_forms():
    g = ref.window()
    assert len(g) == 11 and abs(g.sum() - 1.0) < 1e-15 and np.array_equal(g, g[::-1]) and g[5] == g.max()
    assert g[4] / g[5] == pytest.approx(math.exp(-1.0 / 4.5), rel=1e-14)
    # identical planes give exactly 1 at every scale
    a = ref.textured(3, 180, 190, 8)
    same = ref.ms_ssim_plane(a, a, 8)
    assert same["n_scales"] == 5 and same["cs"] == [1.0] * 5 and same["ssim"] == [1.0] * 5 and same["ms_ssim"] == 1.0
    # a constant offset on a constant plane: no structure to lose (cs = 1), the luminance term by hand
    x = np.full((176, 176), 100, np.uint8)
    y = np.full((176, 176), 110, np.uint8)
    r = ref.ms_ssim_plane(y, x, 8)
    mx, my = 100 / 255.0, 110 / 255.0
    lum = (2 * mx * my + ref.C1) / (mx * mx + my * my + ref.C1)
    assert r["cs"] == pytest.approx([1.0] * 5, abs=1e-12)
    assert r["ssim"] == pytest.approx([lum] * 5, rel=1e-12)
    assert r["ms_ssim"] == pytest.approx(lum ** 0.1333, rel=1e-12)
    # size rule: the shorter side must be at least 176
    assert not ref.enough_for_ms_ssim(175, 4000) and ref.enough_for_ms_ssim(176, 4000) and not ref.enough_for_ms_ssim(4000, 175)
    small = ref.ms_ssim_plane(np.zeros((175, 300), np.uint8), np.zeros((175, 300), np.uint8), 8)
    assert small["n_scales"] == 0 and math.isnan(small["ms_ssim"])
    assert ref.ms_ssim_plane(np.zeros((176, 300), np.uint8), np.zeros((176, 300), np.uint8), 8)["n_scales"] == 5
    # pooling drops a trailing odd row / column
    p = ref.pool2(np.arange(35, dtype=np.float64).reshape(5, 7))
    assert p.shape == (2, 3) and p[0, 0] == (0 + 1 + 7 + 8) / 4.0 and p[1, 2] == (18 + 19 + 25 + 26) / 4.0
    # squared error and PSNR
    d = np.array([[0, 65535]], np.uint16)
    assert ref.sse(d, d[:, ::-1]) == 2 * 65535 ** 2 and ref.psnr([0], [5], 8) == math.inf


# ---- CPU: sources and the results file -----------------------------------------------------------------------------
def _like(h, w, bitdepth, fdt):
    import torch

    from cool_chic_amd.io import FrameData

    if fdt == "yuv420":
        return FrameData(bitdepth, fdt, {"y": torch.zeros(1, 1, h, w), "u": torch.zeros(1, 1, h // 2, w // 2), "v": torch.zeros(1, 1, h // 2, w // 2)})
    return FrameData(bitdepth, fdt, torch.zeros(1, 3, h, w))


@pytest.mark.parametrize("bitdepth", [8, 10, 16])
def test_read_source_ppm_fixtures(bitdepth):
    from cool_chic_amd.quality import read_source

    want = np.load(os.path.join(GOLDEN, "ppm_planes.npz"))[f"ppm{bitdepth}"]
    path = os.path.join(GOLDEN, f"ppm{bitdepth}.ppm")
    fd = read_source(path, _like(5, 7, bitdepth, "rgb"))
    assert fd.bitdepth == bitdepth and fd.frame_data_type == "rgb" and fd.img_size == (5, 7)
    got = fd.integer_planes()
    assert all(np.array_equal(got[c], want[c]) for c in range(3))
    with pytest.raises(ValueError):
        read_source(path, _like(7, 5, bitdepth, "rgb"))
    with pytest.raises(ValueError):
        read_source(path, _like(5, 7, 12, "rgb"))
    with pytest.raises(ValueError):
        read_source(path, _like(5, 7, bitdepth, "yuv444"))


def test_read_source_png_and_yuv(tmp_path):
    from PIL import Image

    from cool_chic_amd.quality import read_source

    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (9, 13, 3), dtype=np.uint8)
    Image.fromarray(img).save(tmp_path / "a.png")
    fd = read_source(str(tmp_path / "a.png"), _like(9, 13, 8, "rgb"))
    assert all(np.array_equal(fd.integer_planes()[c], img[:, :, c]) for c in range(3))
    with pytest.raises(ValueError):
        read_source(str(tmp_path / "a.png"), _like(9, 12, 8, "rgb"))
    with pytest.raises(ValueError):
        read_source(str(tmp_path / "a.png"), _like(9, 13, 10, "rgb"))
    # two 10-bit 4:2:0 frames, two little-endian bytes per sample
    frames = [[rng.integers(0, 1024, s, dtype=np.uint16) for s in ((6, 8), (3, 4), (3, 4))] for _ in range(2)]
    with open(tmp_path / "v.yuv", "wb") as f:
        for fr in frames:
            for p in fr:
                f.write(p.astype("<u2").tobytes())
    like = _like(6, 8, 10, "yuv420")
    for k in range(2):
        fd = read_source(str(tmp_path / "v.yuv"), like, frame_index=k)
        assert fd.frame_data_type == "yuv420" and fd.bitdepth == 10
        assert all(np.array_equal(a, b) for a, b in zip(fd.integer_planes(), frames[k]))
    with pytest.raises(ValueError):
        read_source(str(tmp_path / "v.yuv"), like, frame_index=2)
    with pytest.raises(ValueError):
        read_source(str(tmp_path / "v.yuv"), _like(6, 10, 10, "yuv420"))  # not a whole number of frames of that size
    with pytest.raises(ValueError):
        read_source(str(tmp_path / "v.yuv"), _like(6, 8, 10, "rgb"))
    with pytest.raises(ValueError):
        read_source(str(tmp_path / "v.bmp"), like)


def test_results_file(tmp_path):
    from cool_chic_amd.quality import RESULT_COLUMNS, FrameQuality, write_results

    cs = ((0.9,) * 5,) * 3
    qa = FrameQuality(8, "rgb", (10, 20, 30), (1000, 1000, 1000), (5, 5, 5), cs, cs)
    qb = FrameQuality(8, "rgb", (40, 50, 60), (1000, 1000, 1000), (0, 0, 0), ((),) * 3, ((),) * 3)
    write_results(str(tmp_path / "r.tsv"), [(2, "B", 1000, 50, qb), (0, "I", 1000, 300, qa)], n_bytes_video_header=7)
    lines = (tmp_path / "r.tsv").read_text().splitlines()
    assert lines[0].split("\t") == list(RESULT_COLUMNS)
    assert RESULT_COLUMNS == ("display_index", "frame_type", "n_pixels", "n_bytes", "rate_bpp", "psnr_db", "psnr_0", "psnr_1",
                              "psnr_2", "ms_ssim", "ms_ssim_db")
    rows = [dict(zip(RESULT_COLUMNS, ln.split("\t"))) for ln in lines[1:]]
    assert [r["display_index"] for r in rows] == ["0", "2", "all"] and [r["frame_type"] for r in rows] == ["I", "B", "-"]
    assert float(rows[0]["rate_bpp"]) == 8 * 300 / 1000 and float(rows[1]["rate_bpp"]) == 8 * 50 / 1000
    assert float(rows[0]["psnr_db"]) == qa.psnr_db and float(rows[0]["psnr_2"]) == qa.psnr_planes[2]
    assert float(rows[0]["ms_ssim"]) == qa.ms_ssim and float(rows[0]["ms_ssim_db"]) == qa.ms_ssim_db
    assert math.isnan(float(rows[1]["ms_ssim"])) and math.isnan(float(rows[1]["ms_ssim_db"]))
    # the last row: every byte of the file over every pixel, and the mean of the per-frame values
    assert rows[2]["n_pixels"] == "2000" and rows[2]["n_bytes"] == "357" and float(rows[2]["rate_bpp"]) == 8 * 357 / 2000
    assert float(rows[2]["psnr_db"]) == (qa.psnr_db + qb.psnr_db) / 2 and float(rows[2]["psnr_1"]) == (qa.psnr_planes[1] + qb.psnr_planes[1]) / 2
    assert math.isnan(float(rows[2]["ms_ssim"]))


# ---- GPU -------------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _score(meter, frames, ms_ssim=True, fdts=None):
    """frames: [(dec planes[3], src planes[3], bit depth)] as numpy -> List[FrameQuality]."""
    dec = [[_dev(p) for p in d] for d, _, _ in frames]
    src = [[_dev(p) for p in s] for _, s, _ in frames]
    return meter.score_planes(dec, src, [bd for *_, bd in frames], fdts, ms_ssim)


def _noisy_frame(seed, h, w, bd, ch=None, cw=None, sigma=ref.LIGHT):
    rng = np.random.default_rng(seed)
    dt = np.uint8 if bd == 8 else np.uint16
    sizes = [(h, w), (ch or h, cw or w), (ch or h, cw or w)]
    src = [rng.integers(0, 2 ** bd, s).astype(dt) for s in sizes]
    dec = [ref.with_noise(s, seed + 77 + p, bd, sigma) for p, s in enumerate(src)]
    return dec, src, bd


SSE_SIZES = [(1, 1), (37, 100), (512, 768), (1365, 2048), (2160, 3840)]


@pytest.mark.gpu
@pytest.mark.parametrize("bitdepth", [8, 10, 16])
def test_sse_is_exact(bitdepth):
    from cool_chic_amd.quality import QualityMeter

    frames = [_noisy_frame(100 * bitdepth + i, h, w, bitdepth, sigma=ref.HEAVY) for i, (h, w) in enumerate(SSE_SIZES)]
    frames += [_noisy_frame(900 + bitdepth + i, h, w, bitdepth, h // 2, w // 2) for i, (h, w) in enumerate([(2, 2), (38, 100), (1080, 1920)])]
    fdts = ["rgb"] * len(SSE_SIZES) + ["yuv420"] * 3
    with QualityMeter(0) as meter:
        got = _score(meter, frames, ms_ssim=False, fdts=fdts)
    for (dec, src, bd), q in zip(frames, got):
        want = [ref.sse(d, s) for d, s in zip(dec, src)]
        print(dec[0].shape, bd, "sse", q.sse, "want", want)
        assert list(q.sse) == want and list(q.n) == [d.size for d in dec] and q.n_scales == (0, 0, 0)
        assert q.psnr_db == pytest.approx(ref.psnr(want, q.n, bd), rel=1e-12)
        for p in range(3):
            assert q.psnr_planes[p] == pytest.approx(ref.psnr(want[p:p + 1], q.n[p:p + 1], bd), rel=1e-12)


@pytest.mark.gpu
def test_sse_full_scale_16_bit_and_unaligned_planes():
    import torch

    from cool_chic_amd.quality import QualityMeter

    h, w = 2160, 3840
    zero, full = torch.zeros(h, w, dtype=torch.uint16, device="cuda"), torch.full((h, w), 65535, dtype=torch.uint16, device="cuda")
    # planes that do not start on a 16-byte boundary take the kernel's element-wise path
    rng = np.random.default_rng(4)
    a, b = rng.integers(0, 256, 37 * 101 + 3).astype(np.uint8), rng.integers(0, 256, 37 * 101 + 3).astype(np.uint8)
    da, db = _dev(a), _dev(b)
    ua, ub = da[3:].view(37, 101), db[3:].view(37, 101)
    with QualityMeter(0) as meter:
        q = meter.score_planes([[full, full, zero]], [[zero, zero, zero]], [16], ms_ssim=False)[0]
        u = meter.score_planes([[ua, ua, ua]], [[ub, ub, ua]], [8], ms_ssim=False)[0]
    assert q.sse == (h * w * 65535 ** 2, h * w * 65535 ** 2, 0)  # 3.6e16: beyond float64's integers, inside uint64
    assert q.psnr_planes[0] == 0.0 and q.psnr_planes[2] == math.inf
    want = ref.sse(a[3:], b[3:])
    assert u.sse == (want, want, 0)


def _check_ms(q_planes, dec, src, bd, kind, label):
    """One frame's device means against the float64 restatement; returns the largest deviations (means, ms_ssim)."""
    floor_m, floor_s = ((F32_FLOOR_MEANS_FLAT, F32_FLOOR_MS_SSIM_FLAT) if kind == "flat"
                        else (F32_FLOOR_MEANS_TEXTURED, F32_FLOOR_MS_SSIM_TEXTURED))
    worst_m = worst_s = 0.0
    for p, (d, s) in enumerate(zip(dec, src)):
        want = ref.ms_ssim_plane(d, s, bd)
        assert q_planes.n_scales[p] == want["n_scales"] == 5
        dm = max(abs(a - b) for a, b in zip(list(q_planes.cs[p]) + list(q_planes.ssim[p]), want["cs"] + want["ssim"]))
        ds = abs(q_planes.ms_ssim_planes[p] - want["ms_ssim"])
        print(f"{label} {kind} plane {p}: ms_ssim {q_planes.ms_ssim_planes[p]:.12f} (float64 {want['ms_ssim']:.12f}) "
              f"deviation means {dm:.3e} ms_ssim {ds:.3e}; bound {2 * floor_m:.3e} / {2 * floor_s:.3e}")
        assert dm <= 2 * floor_m and ds <= 2 * floor_s
        worst_m, worst_s = max(worst_m, dm), max(worst_s, ds)
    return worst_m, worst_s


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind", ref.MS_CASES)
def test_ms_ssim_against_float64_restatement(name, kind):
    from cool_chic_amd.quality import QualityMeter

    dec, src, bd = ref.ms_case(name, kind)
    dec3, src3 = (dec * 3)[:3], (src * 3)[:3]  # a one-plane case fills the frame with the same plane
    with QualityMeter(0) as meter:
        q = _score(meter, [(dec3, src3, bd)])[0]
    assert list(q.sse) == [ref.sse(d, s) for d, s in zip(dec3, src3)]
    _check_ms(q, dec3, src3, bd, kind, name)
    assert q.ms_ssim == pytest.approx(sum(q.ms_ssim_planes) / 3.0, rel=1e-15)
    assert q.ms_ssim_db == pytest.approx(ref.ms_ssim_db(q.ms_ssim), rel=1e-12)


def _bits(q):
    return (q.sse, q.n, q.n_scales, tuple(np.float64(v).tobytes() for p in range(3) for v in list(q.cs[p]) + list(q.ssim[p])))


def _mixed_batch():
    """24 frames of mixed sizes, bit depths and formats; some planes are too small for MS-SSIM."""
    shapes = [(512, 768, 8, None), (768, 512, 8, None), (177, 200, 16, None), (540, 960, 10, (270, 480)), (100, 37, 8, None),
              (352, 288, 8, (176, 144)), (1080, 1920, 8, (540, 960)), (176, 176, 12, None)]
    frames, fdts = [], []
    for i in range(24):
        h, w, bd, chroma = shapes[i % len(shapes)]
        frames.append(_noisy_frame(5000 + i, h, w, bd, *(chroma or (None, None)), sigma=ref.LIGHT if i % 2 else ref.HEAVY))
        fdts.append("yuv420" if chroma else "rgb")
    return frames, fdts


@pytest.mark.gpu
def test_deterministic_and_independent_of_the_batch():
    from cool_chic_amd.quality import QualityMeter

    frames, fdts = _mixed_batch()
    with QualityMeter(0) as meter:
        first = _score(meter, frames, fdts=fdts)
        again = _score(meter, frames, fdts=fdts)
        assert [_bits(a) for a in first] == [_bits(b) for b in again]
        # the handle after a larger batch: a frame alone gives the bits it had inside the batch
        for k in (0, 2, 3, 6, 23):
            alone = _score(meter, [frames[k]], fdts=[fdts[k]])[0]
            assert _bits(alone) == _bits(first[k]), f"frame {k} alone differs from frame {k} in the batch"
        tail = _score(meter, frames[5:9][::-1], fdts=fdts[5:9][::-1])[::-1]
        assert [_bits(a) for a in tail] == [_bits(b) for b in first[5:9]]
    with QualityMeter(0) as fresh:
        assert _bits(_score(fresh, [frames[6]], fdts=[fdts[6]])[0]) == _bits(first[6])
    for (dec, src, bd), q in zip(frames, first):
        assert list(q.sse) == [ref.sse(d, s) for d, s in zip(dec, src)]


@pytest.mark.gpu
def test_small_planes_next_to_valid_neighbours():
    from cool_chic_amd.quality import QualityMeter

    frames, fdts = _mixed_batch()
    with QualityMeter(0) as meter:
        got = _score(meter, frames[:8], fdts=fdts[:8])
    for (dec, src, bd), q, fdt in zip(frames[:8], got, fdts[:8]):
        for p in range(3):
            big = ref.enough_for_ms_ssim(*dec[p].shape)
            assert q.n_scales[p] == (5 if big else 0)
            assert math.isnan(q.ms_ssim_planes[p]) != big
    # 100 x 37: nothing; 352 x 288 4:2:0: luma only, and the frame reports the luma
    assert got[4].n_scales == (0, 0, 0) and math.isnan(got[4].ms_ssim) and got[4].psnr_db > 0
    assert got[5].n_scales == (5, 0, 0) and got[5].ms_ssim == got[5].ms_ssim_planes[0]
    _check_ms_planes = [(5, 0), (3, 0), (3, 1), (7, 2)]
    for k, p in _check_ms_planes:
        dec, src, bd = frames[k]
        want = ref.ms_ssim_plane(dec[p], src[p], bd)
        assert abs(got[k].ms_ssim_planes[p] - want["ms_ssim"]) <= 2 * F32_FLOOR_MS_SSIM_TEXTURED


def _write_noisy_png(path, planes, seed):
    from PIL import Image

    noisy = [ref.with_noise(p.astype(np.uint8), seed + k, 8, 0.02) for k, p in enumerate(planes)]
    Image.fromarray(np.stack(noisy, axis=-1)).save(path)
    return noisy


@pytest.mark.gpu
def test_decode_video_scored_kodim14(tmp_path, capsys):
    from cool_chic_amd.bitstream.decode import decode_video, decode_video_scored

    _, z, j = load_golden("kodim14")
    want_planes = [p.astype(np.uint8) for p in reference_planes(z, j)]
    src = _write_noisy_png(str(tmp_path / "src.png"), want_planes, 11)
    cool = os.path.join(GOLDEN, "kodim14.cool")
    plain = decode_video(cool)
    plain_out = capsys.readouterr().out
    frames, qualities = decode_video_scored(cool, str(tmp_path / "src.png"), results_path=str(tmp_path / "r.tsv"))
    assert list(frames) == list(plain) == ["0"] and len(qualities) == 1
    dec = frames["0"].integer_planes()
    assert all(np.array_equal(a, b) for a, b in zip(dec, plain["0"].integer_planes()))
    assert all(int(np.abs(a.astype(np.int32) - b).max()) <= 1 for a, b in zip(dec, want_planes))  # the fixture parity bar
    assert plain_out.startswith("Decoding 1 intra frame(s) time =") and plain_out.count("\n") == 1
    q = qualities[0]
    want = [ref.sse(d, s) for d, s in zip(dec, src)]
    assert list(q.sse) == want and list(q.n) == [512 * 768] * 3
    assert q.psnr_db == pytest.approx(ref.psnr(want, q.n, 8), rel=1e-12)
    ms = [ref.ms_ssim_plane(d, s, 8)["ms_ssim"] for d, s in zip(dec, src)]
    assert q.ms_ssim == pytest.approx(sum(ms) / 3.0, abs=2 * F32_FLOOR_MS_SSIM_TEXTURED)
    rows = [ln.split("\t") for ln in (tmp_path / "r.tsv").read_text().splitlines()]
    assert [r[0] for r in rows] == ["display_index", "0", "all"] and rows[1][1] == "I"
    n_file = os.path.getsize(cool)
    assert int(rows[2][3]) == n_file and 0 < n_file - int(rows[1][3]) < 16  # the video header is in the last row only
    assert float(rows[1][5]) == q.psnr_db and float(rows[2][5]) == q.psnr_db and float(rows[1][9]) == q.ms_ssim
    # decode_video with a source returns what it returns without one
    again = decode_video(cool, source_path=str(tmp_path / "src.png"), ms_ssim=False)
    assert np.array_equal(again["0"].integer_planes()[1], dec[1])


@pytest.mark.gpu
def test_decode_video_scored_vid5_yuv420(tmp_path):
    from cool_chic_amd.bitstream.decode import decode_video_scored

    _, z, j = load_golden("vid5")
    src = {}
    with open(tmp_path / "src.yuv", "wb") as f:
        for d in range(5):
            src[d] = [ref.with_noise(p.astype(np.uint8), 300 + 3 * d + k, 8, 0.03) for k, p in enumerate(reference_planes(z, j, str(d)))]
            for p in src[d]:
                f.write(p.tobytes())
    frames, qualities = decode_video_scored(os.path.join(GOLDEN, "vid5.cool"), str(tmp_path / "src.yuv"), results_path=str(tmp_path / "r.tsv"))
    assert len(qualities) == 5
    for d in range(5):
        dec = frames[str(d)].integer_planes()
        want = [ref.sse(a, b) for a, b in zip(dec, src[d])]
        q = qualities[d]
        assert list(q.sse) == want and q.n[1] * 4 == q.n[0]
        assert q.psnr_db == pytest.approx(ref.psnr(want, q.n, 8), rel=1e-12)
        assert q.n_scales == (0, 0, 0) and math.isnan(q.ms_ssim)
    rows = [ln.split("\t") for ln in (tmp_path / "r.tsv").read_text().splitlines()]
    assert [r[0] for r in rows[1:]] == ["0", "1", "2", "3", "4", "all"]
    assert rows[1][1] == "I" and set(r[1] for r in rows[2:6]) <= {"P", "B"} and all(r[9] == "nan" and r[10] == "nan" for r in rows[1:])
    assert int(rows[6][3]) == os.path.getsize(os.path.join(GOLDEN, "vid5.cool"))
    assert float(rows[6][5]) == pytest.approx(sum(q.psnr_db for q in qualities) / 5.0, rel=1e-15)


@pytest.mark.gpu
def test_decode_video_scored_synthetic_1080p_gop(tmp_path):
    from cool_chic_amd import synth
    from cool_chic_amd.bitstream.decode import decode_video, decode_video_scored

    stream, _ = synth.gop1080p(intra_period=2)
    (tmp_path / "gop.cool").write_bytes(stream)
    plain = decode_video(str(tmp_path / "gop.cool"))
    src = {}
    with open(tmp_path / "src.yuv", "wb") as f:
        for d in range(3):
            src[d] = [ref.with_noise(p, 700 + 3 * d + k, 8, 0.02) for k, p in enumerate(plain[str(d)].integer_planes())]
            for p in src[d]:
                f.write(p.tobytes())
    frames, qualities = decode_video_scored(str(tmp_path / "gop.cool"), str(tmp_path / "src.yuv"))
    for d in range(3):
        dec = frames[str(d)].integer_planes()
        assert dec[0].shape == (1080, 1920) and dec[1].shape == (540, 960)
        assert all(np.array_equal(a, b) for a, b in zip(dec, plain[str(d)].integer_planes()))
        q = qualities[d]
        want = [ref.sse(a, b) for a, b in zip(dec, src[d])]
        assert list(q.sse) == want and q.psnr_db == pytest.approx(ref.psnr(want, q.n, 8), rel=1e-12)
        assert q.n_scales == (5, 5, 5)
        luma = ref.ms_ssim_plane(dec[0], src[d][0], 8)["ms_ssim"]
        print(f"frame {d}: psnr {q.psnr_db:.4f} dB ms_ssim {q.ms_ssim:.9f} (float64 {luma:.9f})")
        assert q.ms_ssim == q.ms_ssim_planes[0] and abs(q.ms_ssim - luma) <= 2 * F32_FLOOR_MS_SSIM_TEXTURED


@pytest.mark.gpu
def test_cc_decode_command_line(tmp_path):
    _, z, j = load_golden("kodim14")
    want_planes = [p.astype(np.uint8) for p in reference_planes(z, j)]
    src = _write_noisy_png(str(tmp_path / "src.png"), want_planes, 23)
    base = [sys.executable, os.path.join(ROOT, "cc_decode.py"), "-i", os.path.join(GOLDEN, "kodim14.cool")]
    plain = subprocess.run(base + ["-o", str(tmp_path / "plain.ppm")], capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0, plain.stderr
    scored = subprocess.run(base + ["-o", str(tmp_path / "scored.ppm"), "--source", str(tmp_path / "src.png"), "--results",
                                    str(tmp_path / "r.tsv"), "--no-ms-ssim"], capture_output=True, text=True, timeout=600)
    assert scored.returncode == 0, scored.stderr
    assert (tmp_path / "plain.ppm").read_bytes() == (tmp_path / "scored.ppm").read_bytes()
    assert plain.stdout.startswith("Decoding 1 intra frame(s) time =") and plain.stdout.count("\n") == 1
    rows = [ln.split("\t") for ln in (tmp_path / "r.tsv").read_text().splitlines()]
    from cool_chic_amd.quality import _read_ppm

    dec, _ = _read_ppm(str(tmp_path / "scored.ppm"))  # what the child process decoded
    want = [ref.sse(d, s) for d, s in zip(dec, src)]
    assert float(rows[1][5]) == pytest.approx(ref.psnr(want, [512 * 768] * 3, 8), rel=1e-12)
    assert rows[1][9] == "nan" and rows[2][0] == "all"
    bad = subprocess.run(base + ["--results", str(tmp_path / "x.tsv")], capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "--results needs --source" in bad.stderr
