"""PNG packer level 1: LZ77 matches searched on the device inside every deflate block.

The canon is restated on the CPU in tests/png_lz77_ref.py.  The bar: the device bytes equal the restatement's, every
reader gets the exact planes back, a level-1 file is never larger than the level-0 file, and on the Kodak fixture it is
within 4 % of PIL's (zlib level 6, the reference's writer)."""
import io
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import png_lz77_ref as R
from png_pictures import SIZES, _deep_litlen_row, _pictures, _read_png, _unlimited_depths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CCD_ERR_ARG = -7


def _idat(png: bytes) -> bytes:
    pos, data = 8, b""
    while pos < len(png):
        n, kind = struct.unpack(">I4s", png[pos:pos + 8])
        if kind == b"IDAT":
            data += png[pos + 8:pos + 8 + n]
        pos += 12 + n
    return data


def _scanlines(planes) -> bytes:
    from oracle import png_pack

    scan, _ = png_pack.filter_rows(np.ascontiguousarray(planes.transpose(1, 2, 0)))
    return scan.tobytes()


def _pil_size(planes) -> int:
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(planes.transpose(1, 2, 0))).save(b, format="PNG")
    return len(b.getvalue())


def _kodim14():
    from conftest import load_golden, reference_planes

    _, z, j = load_golden("kodim14")
    return np.stack(reference_planes(z, j)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ CPU: the C ABI
def test_set_level_rejects_bad_arguments():
    from cool_chic_amd import _lib

    L = _lib.lib()
    assert L.ccd_png_set_level(None, 1) == CCD_ERR_ARG
    assert L.ccd_png_set_level(None, 5) == CCD_ERR_ARG
    assert L.ccd_png_set_level(None, 0) == CCD_ERR_ARG


# ------------------------------------------------------------------------------------------------ CPU: the restatement
def test_code_lengths_generalise_the_oracle():
    from oracle import png_pack

    rng = np.random.default_rng(3)
    for _ in range(20):
        hist = rng.integers(0, 50, 257) * rng.integers(0, 2, 257)
        hist[256] = 1
        hist[rng.integers(0, 256)] += 1
        assert np.array_equal(R.code_lengths(hist), png_pack.code_lengths(hist))
    # all 286 lit/len symbols used with geometric counts: limited to 15 bits, complete
    hist = np.maximum(1, (1e6 * 0.7 ** np.arange(286)).astype(np.int64))
    lens = R.code_lengths(hist)
    assert lens.max() == 15 and sum(2.0 ** -int(v) for v in lens) == 1.0
    one = np.zeros(30, np.int64)
    one[7] = 12
    assert list(np.nonzero(R.code_lengths(one))[0]) == [7] and R.code_lengths(one)[7] == 1
    assert not R.code_lengths(np.zeros(30, np.int64)).any()


@pytest.mark.parametrize("h,w", SIZES)
def test_restatement_round_trips_and_never_grows(h, w):
    from oracle import png_pack

    for kind, planes in _pictures(h, w).items():
        info = []
        png = R.pack_rgb8(planes, info=info)
        level0 = png_pack.pack_rgb8(planes)
        assert zlib.decompress(_idat(png)) == _scanlines(planes), (h, w, kind)
        assert np.array_equal(_read_png(png), planes), (h, w, kind)
        assert len(png) <= len(level0), (h, w, kind)
        if kind == "random":  # no block gains from matches: every block falls back to the level-0 coding
            assert png == level0 and all(c == "lit" for _, c in info), (h, w)


def test_overlapping_run_at_distance_one():
    data = np.full(100, 5, np.uint8)
    pos, L, D = R.parse(*R.matches(data))
    assert list(pos) == [0, 1] and list(L) == [0, 99] and list(D) == [0, 1]


def test_match_capped_at_258():
    data = np.zeros(1000, np.uint8)
    data[0] = 1
    mlen, mdist = R.matches(data)
    assert mlen[2] == 258 and mdist[2] == 1 and mlen.max() == 258
    pos, L, D = R.parse(mlen, mdist)
    assert list(L[:4]) == [0, 0, 258, 258] and set(D[L > 0]) == {1}


def test_window_of_32768_inside_one_16383_wide_row():
    """One row of 16383 pixels is one block of 49150 bytes: a repeat at distance 32769 is out of the window, one at
    32768 is used."""
    from oracle import png_pack

    n = 3 * 16383 + 1
    assert png_pack.rows_per_block(16383) == 1
    rng = np.random.default_rng(5)
    seg_a = rng.integers(0, 128, 20).astype(np.uint8)
    seg_b = rng.integers(0, 128, 20).astype(np.uint8)
    a, b = 1000, 5000
    ta, tb = R.buckets(seg_a[:3])[0], R.buckets(seg_b[:3])[0]
    assert ta != tb
    starts = {a, a + 32769, b, b + 32768}
    data = rng.integers(128, 256, n).astype(np.uint8)  # background bytes never equal segment bytes
    for _ in range(100):
        for s, seg in ((a, seg_a), (a + 32769, seg_a), (b, seg_b), (b + 32768, seg_b)):
            data[s:s + 20] = seg
        hit = [i for i in np.nonzero(np.isin(R.buckets(data), [ta, tb]))[0] if i not in starts]
        if not hit:
            break
        for i in hit:  # re-draw a background byte of the colliding key
            k = next(q for q in range(i, i + 3) if data[q] >= 128)
            data[k] = rng.integers(128, 256)
    assert not hit
    for dst, src in ((a + 32769 + 20, a + 20), (b + 32768 + 20, b + 20)):  # the copies end where their sources end
        data[dst] = 128 if data[src] != 128 else 129
    mlen, mdist = R.matches(data)
    assert mlen[a + 32769] == 0
    assert mlen[b + 32768] == 20 and mdist[b + 32768] == 32768
    pos, L, D = R.parse(mlen, mdist)
    assert D.max() <= 32768
    k = int(np.searchsorted(pos, b + 32768))
    assert pos[k] == b + 32768 and L[k] == 20 and D[k] == 32768


def test_block_with_a_single_distance_symbol():
    from oracle import png_pack

    planes = np.zeros((3, 64, 64), np.uint8)
    scan, _ = png_pack.filter_rows(planes.transpose(1, 2, 0))
    data = scan.reshape(-1)
    bits, (lens_ll, lens_d, *_), (pos, L, D) = R.lz77_block(data)
    assert set(D[L > 0]) == {1}
    assert list(np.nonzero(lens_d)[0]) == [0] and lens_d[0] == 1
    info = []
    png = R.pack_rgb8(planes, info=info)
    assert [c for _, c in info] == ["lz"]
    assert np.array_equal(_read_png(png), planes)
    assert zlib.decompress(_idat(png)) == data.tobytes()


def test_lazy_rule_takes_the_longer_match_one_byte_later():
    data = np.array([10, 11, 12, 99, 11, 12, 13, 14, 15, 16, 98, 10, 11, 12, 13, 14, 15, 16, 97], np.uint8)
    mlen, mdist = R.matches(data)
    assert (mlen[11], mdist[11]) == (3, 11) and (mlen[12], mdist[12]) == (6, 8)
    pos, L, D = R.parse(mlen, mdist)
    k = list(pos).index(11)
    assert (L[k], pos[k + 1], L[k + 1], D[k + 1]) == (0, 12, 6, 8)  # a literal at 11, then the longer match
    assert pos[k + 2] == 18


def test_kodak_size_against_pil():
    from oracle import png_pack

    planes = _kodim14()
    png = R.pack_rgb8(planes)
    assert np.array_equal(_read_png(png), planes)
    assert len(png) <= 1.04 * _pil_size(planes)
    assert len(png) < len(png_pack.pack_rgb8(planes))


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def packer():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cool_chic_amd.io.png import PngPacker

    p = PngPacker(0, level=1)
    yield p
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", SIZES)
def test_device_level1_equals_restatement(packer, h, w):
    import torch

    for kind, planes in _pictures(h, w).items():
        png = packer.pack(torch.from_numpy(planes).cuda())
        assert np.array_equal(_read_png(png), planes), (h, w, kind)
        assert png == R.pack_rgb8(planes), (h, w, kind)


@pytest.mark.gpu
def test_device_png_lz77_of_a_litlen_tree_deeper_than_15_bits(packer):
    """No other byte-compared picture has a block that takes the LZ77 coding with a literal/length tree deeper than 15 bits
    (their deepest is 12): here the fold to 15 bits and the Kraft repair run on the 286-symbol alphabet and show."""
    import torch

    from oracle import png_pack

    planes = _deep_litlen_row()
    data = np.frombuffer(_scanlines(planes), np.uint8)
    assert planes.shape[1] == 1 and data[0] == 1  # one row = one block, Sub filter
    _, (lens_ll, *_), (pos, L, _) = R.lz77_block(data)
    sym = np.where(L == 0, data[pos].astype(np.int64), R.len_sym(np.where(L == 0, 3, L))[0])
    hll = np.bincount(sym, minlength=R.NLL)
    hll[256] += 1
    assert _unlimited_depths(R.code_lengths, hll).max() > png_pack.MAX_BITS
    assert lens_ll.max() == png_pack.MAX_BITS
    info = []
    want = R.pack_rgb8(planes, info=info)
    assert [c for _, c in info] == ["lz"]
    png = packer.pack(torch.from_numpy(planes).cuda())
    assert np.array_equal(_read_png(png), planes)
    assert png == want


@pytest.mark.gpu
def test_device_level1_batch_and_wide_rows(packer):
    import torch

    pics = [_pictures(h, w)[kind] for (h, w), kind in zip(SIZES + [(300, 200), (64, 512)],
                                                         ["random", "smooth", "photo", "zeros", "skewed"] * 2)]
    pics += [_pictures(1, 16383)["photo"], _pictures(2, 16383)["smooth"], _pictures(2, 16383)["skewed"], _kodim14()]
    got = packer.pack_many([torch.from_numpy(p).cuda() for p in pics])
    for p, png in zip(pics, got):
        assert np.array_equal(_read_png(png), p)
        assert png == R.pack_rgb8(p), p.shape
    for h, w in ((1, 16383), (2, 16383)):
        for kind, planes in _pictures(h, w).items():
            png = packer.pack(torch.from_numpy(planes).cuda())
            assert np.array_equal(_read_png(png), planes), (h, w, kind)
            assert png == R.pack_rgb8(planes), (h, w, kind)


@pytest.mark.gpu
def test_device_level1_4k_round_trips(packer):
    import torch

    from cool_chic_amd.io.png import PngPacker

    planes = torch.from_numpy(_pictures(2160, 3840)["photo"]).cuda()
    png = packer.pack(planes)
    assert np.array_equal(_read_png(png), planes.cpu().numpy())
    p0 = PngPacker(0)
    try:
        assert len(png) <= len(p0.pack(planes))
    finally:
        p0.close()


@pytest.mark.gpu
def test_levels_share_a_handle_without_leaking_state():
    import torch

    from cool_chic_amd.io.png import PngPacker
    from oracle import png_pack

    planes = _kodim14()
    d = torch.from_numpy(planes).cuda()
    p = PngPacker(0, level=1)
    try:
        first = p.pack(d)
        p.set_level(0)
        assert p.pack(d) == png_pack.pack_rgb8(planes)
        p.set_level(1)
        assert p.pack(d) == first == R.pack_rgb8(planes)
        with pytest.raises(ValueError):
            p.set_level(2)
        # the C ABI itself rejects a bad level on a live handle, and the handle keeps its level
        from cool_chic_amd._lib import lib

        for bad in (2, 5, -1):
            assert lib().ccd_png_set_level(p._h, bad) == CCD_ERR_ARG
        assert p.pack(d) == first
    finally:
        p.close()


@pytest.mark.gpu
def test_cc_decode_png_level(tmp_path):
    out = {}
    for level in (0, 1):
        path = str(tmp_path / f"l{level}.png")
        subprocess.run([sys.executable, os.path.join(ROOT, "cc_decode.py"), "-i", os.path.join(ROOT, "tests", "golden", "kodim14.cool"),
                        "-o", path, "--png-level", str(level)], cwd=ROOT, check=True, timeout=300)
        with open(path, "rb") as f:
            out[level] = f.read()
    p0, p1 = _read_png(out[0]), _read_png(out[1])
    assert np.array_equal(p0, p1)
    assert len(out[1]) <= 1.04 * _pil_size(p1)
    assert len(out[1]) < len(out[0])
