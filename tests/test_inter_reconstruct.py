"""P / B frame reconstruction (ccd_inter.hip through ccd_inter_reconstruct / ccd_decode_video) away from the one operating point
of the reference-encoded video fixtures (8-bit 4:2:0, 128 x 224, warp filters 2 / 4 / 8): every even filter size 2..16, bit
depths 8..16, RGB / 4:2:0 / 4:4:4, pictures that leave partial 64 x 4 blocks or are one pixel wide, flows from zero to far
beyond the picture and beyond 2^31, non-finite flows.

Three parties: the CPU oracle (ora_inter_reconstruct, float32, the canon the kernel must match bit for bit), the HIP kernel,
and tests/inter_reference.py - a float64 restatement of what the reference does, which shares no float formula with the other
two.  The CPU tests hold the oracle to the float64 reference; the GPU tests hold the kernel to the oracle (bit-exact, 16-bit
planes included, where a one-ulp change of the blend shows) and a subset to the float64 reference."""
import ctypes as C
from typing import NamedTuple

import numpy as np
import pytest

import inter_reference
from conftest import load_golden

FILTER_SIZES = [2, 4, 6, 8, 10, 12, 14, 16]
FORMATS = {0: "rgb", 1: "yuv420", 2: "yuv444"}
PAIRS = [(bd, fdt) for bd in (8, 9, 10, 12, 16) for fdt in FORMATS]  # every (bit depth, format)
FINITE_FLOWS = ["zero", "integer", "half_integer", "subpixel", "negative_floor", "beyond_picture", "1e4", "1e6", "3e9", "1e10",
                "signed_zero_subnormal"]
NONFINITE_FLOWS = ["nonfinite"]
# partial 64 x 4 blocks (37 x 53, 5 x 130, 67 x 200), small pictures, one row / one column (sinc sizes only: the grid_sample
# warps divide by (n - 1) / 2); 4:2:0 rounds every side up to even
SHAPES = [(37, 53), (5, 130), (67, 200), (9, 31), (1, 77), (45, 1), (16, 24), (3, 66)]
CCD_ERR_VALUE, CCD_ERR_HIP, CCD_ERR_ARG = -2, -6, -7


def _flows(cls, h, w, rng):
    """(fx, fy) float32 [h][w] of one flow class"""
    shape = (h, w)
    sign = lambda: rng.choice([-1.0, 1.0], size=shape)  # noqa: E731
    sub = lambda: rng.uniform(-3.0, 3.0, size=shape)  # noqa: E731
    if cls == "zero":
        fx = fy = np.zeros(shape)
    elif cls == "integer":  # d == 0 in one tap of the sinc window
        fx, fy = rng.integers(-5, 6, size=shape).astype(np.float64), rng.integers(-5, 6, size=shape).astype(np.float64)
    elif cls == "half_integer":
        fx, fy = rng.integers(-5, 5, size=shape) + 0.5, rng.integers(-5, 5, size=shape) + 0.5
    elif cls == "subpixel":
        fx, fy = sub(), sub()
    elif cls == "negative_floor":  # floor crosses zero: -1 for (-1, 0), -2 for (-2, -1)
        fx, fy = -rng.uniform(1e-3, 2.0, size=shape), -rng.uniform(1e-3, 2.0, size=shape)
    elif cls == "signed_zero_subnormal":
        vals = np.array([-0.0, 0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 1.1754942e-38, -1.1754942e-38], dtype=np.float32)
        fx, fy = rng.choice(vals, size=shape), rng.choice(vals, size=shape)
    elif cls == "nonfinite":
        vals = np.array([np.inf, -np.inf, np.nan, 0.5, -2.25, 3e9, -1e10], dtype=np.float32)
        fx, fy = rng.choice(vals, size=shape), rng.choice(vals, size=shape)
    else:  # far away: per pixel the x, the y or both components large, the other a sub-pixel flow
        mag = {"beyond_picture": None, "1e4": 1e4, "1e6": 1e6, "3e9": 3e9, "1e10": 1e10}[cls]
        bx = (w + 100.0) + rng.uniform(0, 1, size=shape) if mag is None else mag * (1.0 + rng.uniform(0, 0.01, size=shape))
        by = (h + 100.0) + rng.uniform(0, 1, size=shape) if mag is None else mag * (1.0 + rng.uniform(0, 0.01, size=shape))
        which = rng.integers(0, 3, size=shape)
        fx = np.where(which != 1, sign() * bx, sub())
        fy = np.where(which != 0, sign() * by, sub())
    return np.asarray(fx, np.float32), np.asarray(fy, np.float32)


def _global_flows(k, h, w):
    """0, small, beyond the picture; different per reference"""
    return [[0, 0, 0, 0], [1, -2, -3, 1], [w + 5, -(h + 7), -(w + 9), h + 3], [-2, 1, 0, 0], [0, 0, 2, -1]][k % 5]


def make_cases(flow_classes):
    """The case list: every filter size meets every flow class and every (bit depth, format) pair; P and B alternate.
    Seeded: the same list on every machine."""
    cases = []
    for fi, n in enumerate(FILTER_SIZES):
        for k in range(max(len(flow_classes), len(PAIRS))):
            bd, fdt = PAIRS[(k + 4 * fi) % len(PAIRS)]
            cls = flow_classes[k % len(flow_classes)]
            ft = 1 + (k + fi) % 2
            h, w = SHAPES[(k + 3 * fi) % len(SHAPES)]
            if n < 6 and min(h, w) == 1:
                h, w = 9, 31
            if fdt == 1:
                h, w = h + h % 2, w + w % 2
            cases.append(dict(id=f"n{n}-{'PB'[ft - 1]}-{bd}bit-{FORMATS[fdt]}-{h}x{w}-{cls}", n_taps=n, frame_type=ft, bitdepth=bd,
                              fdt=fdt, h=h, w=w, flow=cls, gflow=_global_flows(k + fi, h, w), seed=1000 * fi + k))
    return cases


def case_data(c):
    """residue, motion, reference planes of one case"""
    rng = np.random.default_rng(c["seed"])
    h, w, ft, maxv = c["h"], c["w"], c["frame_type"], 2 ** c["bitdepth"] - 1
    n_refs = 2 if ft == 2 else 1
    res = rng.uniform(-0.15, 0.15, size=(3 + n_refs, h, w))
    push = rng.random((3, h, w)) < 0.1  # residues that push samples out of [0, 1]
    res[:3] = np.where(push, rng.choice([-1.0, 1.0], size=(3, h, w)) * rng.uniform(0.6, 1.0, size=(3, h, w)), res[:3])
    res[3:] = rng.uniform(-1.0, 1.0, size=(n_refs, h, w))  # alpha / beta inside and outside [-0.5, 0.5]
    mot = np.concatenate([np.stack(_flows(c["flow"], h, w, rng)) for _ in range(n_refs)])
    ch, cw = (h // 2, w // 2) if c["fdt"] == 1 else (h, w)
    refs = [[rng.integers(0, maxv + 1, size=s).astype(np.uint16) for s in ((h, w), (ch, cw), (ch, cw))] for _ in range(n_refs)]
    return res.astype(np.float32), mot.astype(np.float32), refs[0], (refs[1] if n_refs == 2 else None)


CASES = make_cases(FINITE_FLOWS)
GPU_CASES = make_cases(FINITE_FLOWS + NONFINITE_FLOWS)
# Fraction of samples 1 LSB away from the float64 reference, as measured on the oracle (with saturated sinc indices) for CASES and
# for the GPU test's subset CASES[::3]: bars, not to be raised to let a run pass
F64_MISMATCH_ALL = 1513 / 668160
F64_MISMATCH_SUBSET = 408 / 226542


def _oracle(oracle, c, d):
    res, mot, r0, r1 = d
    return oracle.inter_reconstruct(c["frame_type"], res, mot, r0, r1, c["gflow"], c["n_taps"], c["bitdepth"], c["fdt"])


def _f64(c, d):
    res, mot, r0, r1 = d
    return inter_reference.inter_reconstruct(c["frame_type"], res, mot, r0, r1, c["gflow"], c["n_taps"], c["bitdepth"], c["fdt"])


def _compare_to_f64(cases, run):
    """(bad cases [(id, max |diff|)], mismatching samples, samples) of run(case, data) against the float64 reference"""
    bad, n_diff, n_tot = [], 0, 0
    for c in cases:
        d = case_data(c)
        got, want = run(c, d), _f64(c, d)
        dmax = 0
        for g, wv in zip(got, want):
            diff = np.abs(g.astype(np.int64) - wv)
            dmax = max(dmax, int(diff.max()))
            n_diff += int((diff != 0).sum())
            n_tot += diff.size
        if dmax > 1:
            bad.append((c["id"], dmax))
    return bad, n_diff, n_tot


def test_case_list_covers_every_combination():
    for cases, classes in ((CASES, FINITE_FLOWS), (GPU_CASES, FINITE_FLOWS + NONFINITE_FLOWS)):
        for n in FILTER_SIZES:
            mine = [c for c in cases if c["n_taps"] == n]
            assert {c["flow"] for c in mine} == set(classes)
            assert {(c["bitdepth"], c["fdt"]) for c in mine} == set(PAIRS)
            assert {c["frame_type"] for c in mine} == {1, 2}
            if n >= 6:
                assert any(c["h"] == 1 or c["w"] == 1 for c in mine)
            assert any(c["h"] % 4 and c["w"] % 64 for c in mine)  # partial blocks in both directions
        assert all(c["h"] % 2 == 0 and c["w"] % 2 == 0 for c in cases if c["fdt"] == 1)


def test_oracle_matches_float64_reference(oracle):
    """The oracle's float32 reconstruction against the float64 restatement: every sample within 1 LSB, at every bit depth."""
    bad, n_diff, n_tot = _compare_to_f64(CASES, lambda c, d: _oracle(oracle, c, d))
    assert not bad, f"{len(bad)} cases beyond 1 LSB of the float64 reference: {bad[:8]}"
    # measured on the oracle with saturated sinc indices: 1 513 of 668 160 samples = 0.002264, most of them 4:2:0 chroma, where
    # the 2 x 2 mean of samples on the bit-depth grid is a rounding tie that float32 and float64 break differently
    assert n_diff / n_tot <= F64_MISMATCH_ALL, f"{n_diff} of {n_tot} samples differ by 1 LSB"


def test_oracle_reconstruct_is_the_decode_video_chain(oracle):
    """ora_decode_video reconstructs P / B frames through ora_inter_reconstruct: the planes of a fixture's B frame, rebuilt from
    its two cool-chics and its references, equal the decoded frame."""
    bs, _, _ = load_golden("vid5")
    frames = oracle.decode_video(bs)
    _, coded = oracle.split_stream(bs)
    fh, ccs = coded[2]
    assert fh.frame_type == 2
    res = oracle.decode_coolchic(*ccs[0])["out"]
    mot = oracle.decode_coolchic(*ccs[1])["out"]
    refs = [frames[fh.index_references[k]]["planes"] for k in range(2)]
    got = oracle.inter_reconstruct("B", res, mot, refs[0], refs[1], list(fh.global_flow), fh.warp_filter_size, fh.bitdepth,
                                   fh.frame_data_type)
    for g, w in zip(got, frames[fh.display_index]["planes"]):
        assert np.array_equal(g, w)


def _invalid_calls():
    """(label, keyword changes to a valid call, expected C ABI code)"""
    return [("yuv420_odd_h", dict(h=7, fdt=1), CCD_ERR_VALUE), ("yuv420_odd_w", dict(w=9, fdt=1), CCD_ERR_VALUE),
            ("yuv420_odd_both", dict(h=7, w=9, fdt=1), CCD_ERR_VALUE),
            ("filter_0", dict(n_taps=0), CCD_ERR_VALUE), ("filter_1", dict(n_taps=1), CCD_ERR_VALUE),
            ("filter_3", dict(n_taps=3), CCD_ERR_VALUE), ("filter_18", dict(n_taps=18), CCD_ERR_VALUE),
            ("format_4", dict(fdt=4), CCD_ERR_VALUE), ("format_-1", dict(fdt=-1), CCD_ERR_VALUE),
            ("bitdepth_7", dict(bitdepth=7), CCD_ERR_ARG), ("bitdepth_17", dict(bitdepth=17), CCD_ERR_ARG),
            ("b_without_ref1", dict(frame_type=2, ref1=False), CCD_ERR_ARG)]


def test_inter_reconstruct_rejects_invalid_arguments():
    """ccd_inter_reconstruct validates before it touches a device: device = -1, so that a call that got past the checks fails
    in hipSetDevice (CCD_ERR_HIP) instead of launching anything.  The host buffers below are never read."""
    from cool_chic_amd._lib import lib

    buf = np.zeros(64, np.float32)
    planes = (C.c_void_p * 3)(*[buf.ctypes.data] * 3)
    gf = (C.c_int32 * 4)(0, 0, 0, 0)
    base = dict(frame_type=1, h=8, w=10, bitdepth=10, fdt=1, n_taps=8, ref1=True)

    def call(**kw):
        a = {**base, **kw}
        return lib().ccd_inter_reconstruct(-1, None, a["frame_type"], a["h"], a["w"], a["bitdepth"], a["fdt"],
                                           C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data), planes,
                                           planes if a["ref1"] else None, gf, a["n_taps"], planes)

    assert call() == CCD_ERR_HIP, "a valid call must get as far as hipSetDevice(-1)"
    assert call(frame_type=2) == CCD_ERR_HIP
    assert call(fdt=3, h=7, w=9) == CCD_ERR_HIP  # odd sizes are fine outside 4:2:0
    for label, kw, code in _invalid_calls():
        assert call(**kw) == code, label


def test_oracle_rejects_invalid_arguments(oracle):
    """ora_inter_reconstruct validates the same arguments as the C ABI."""
    for label, kw, _code in _invalid_calls():
        if label == "b_without_ref1":
            continue  # the numpy wrapper refuses the missing buffers itself
        a = {**dict(frame_type=1, h=8, w=10, bitdepth=10, fdt=1, n_taps=8), **kw}
        h, w = a["h"], a["w"]
        ch, cw = (h // 2, w // 2) if a["fdt"] == 1 else (h, w)
        ref = [np.zeros((h, w), np.uint16), np.zeros((ch, cw), np.uint16), np.zeros((ch, cw), np.uint16)]
        with pytest.raises(oracle.OracleError) as e:
            oracle.inter_reconstruct(a["frame_type"], np.zeros((4, h, w), np.float32), np.zeros((2, h, w), np.float32), ref, None,
                                     [0, 0], a["n_taps"], a["bitdepth"], a["fdt"])
        assert e.value.code == -2, label  # ORA_ERR_VALUE


# ---------------------------------------------------------------------------------------------------------------- GPU


class _Inputs(NamedTuple):
    """The device tensors of one call: the two float outputs, the planes of one or two references, the planes it writes."""
    residue: object
    motion: object
    refs: list
    out: list


def _device_inputs(c, d):
    import torch

    res, mot, r0, r1 = d
    dev = torch.device("cuda:0")
    dt = torch.uint8 if c["bitdepth"] == 8 else torch.uint16

    def planes(ps):
        return [torch.from_numpy(p.astype(np.int32)).to(dev).to(dt).contiguous() for p in ps]

    refs = [planes(r0)] + ([planes(r1)] if r1 is not None else [])
    out = [torch.zeros(p.shape, dtype=dt, device=dev) for p in r0]
    return _Inputs(torch.from_numpy(res).to(dev).contiguous(), torch.from_numpy(mot).to(dev).contiguous(), refs, out)


def _launch(c, t, stream):
    """ccd_inter_reconstruct of the case over the tensors `t` on `stream` (a hipStream_t as an integer, 0: the default stream)."""
    from cool_chic_amd._lib import check, lib

    def ptrs(ps):
        return (C.c_void_p * 3)(*[p.data_ptr() for p in ps])

    gf = (C.c_int32 * 4)(*c["gflow"])
    check(lib().ccd_inter_reconstruct(0, C.c_void_p(stream or None), c["frame_type"], c["h"],
                                      c["w"], c["bitdepth"], c["fdt"], C.c_void_p(t.residue.data_ptr()), C.c_void_p(t.motion.data_ptr()),
                                      ptrs(t.refs[0]), ptrs(t.refs[1]) if len(t.refs) == 2 else None, gf, c["n_taps"], ptrs(t.out)),
          "ccd_inter_reconstruct")


def _kernel(c, d, stream=None):
    """The planes the kernel writes for the case; `stream`: a hipStream_t as an integer, torch's current stream by default."""
    import torch

    t = _device_inputs(c, d)
    torch.cuda.synchronize()
    _launch(c, t, torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream if stream is None else stream)
    return [p.to(torch.int32).cpu().numpy().astype(np.uint16) for p in t.out]


@pytest.mark.gpu
def test_kernel_matches_oracle(oracle):
    """ccd_inter_reconstruct against the oracle, bit-exact, over every case - non-finite flows included."""
    import torch

    assert torch.cuda.is_available(), "this test needs the MI355X"
    bad = []
    for c in GPU_CASES:
        d = case_data(c)
        got, want = _kernel(c, d), _oracle(oracle, c, d)
        n = sum(int((g != w).sum()) for g, w in zip(got, want))
        if n:
            bad.append((c["id"], n))
    assert not bad, f"{len(bad)} of {len(GPU_CASES)} cases differ from the oracle (case, samples): {bad[:10]}"


@pytest.mark.gpu
def test_kernel_matches_float64_reference():
    """A subset (every third case) of the kernel's results against the float64 reference, with the CPU test's bar: guards against
    a mistake the kernel and the oracle share."""
    import torch

    assert torch.cuda.is_available(), "this test needs the MI355X"
    bad, n_diff, n_tot = _compare_to_f64(CASES[::3], _kernel)
    assert not bad, f"{len(bad)} cases beyond 1 LSB of the float64 reference: {bad[:8]}"
    # the oracle's value on this subset, measured: 408 of 226 542 samples = 0.001801
    assert n_diff / n_tot <= F64_MISMATCH_SUBSET, f"{n_diff} of {n_tot} samples differ by 1 LSB"


def _rewrite_vid5(fdt, bitdepth, n_taps, motion_edit=None):
    """vid5 with every frame header rewritten to (format, bit depth, warp filter size); motion_edit = (coding index, stream bytes
    of a replacement motion cool-chic) swaps one P / B frame's motion cool-chic."""
    from cool_chic_amd import writer
    from oracle import oracle_py as oracle

    bs, _, _ = load_golden("vid5")
    vh, frames = oracle.split_stream(bs)
    out = [writer.video_header_bytes(vh.n_frames, list(vh.intra_pos[:vh.n_intras]), list(vh.p_pos[:vh.n_p_frames]))]
    for f, (fh, ccs) in enumerate(frames):
        out.append(writer.frame_header_bytes(fh.display_index, "IPB"[fh.frame_type], fdt, bitdepth, list(fh.index_references[:fh.n_refs]),
                                             list(fh.global_flow[:2 * fh.n_refs]), n_taps if fh.frame_type else 0))
        for i, triple in enumerate(ccs):
            out.append(motion_edit[1] if motion_edit and motion_edit[0] == f and i == 1 else b"".join(triple))
    return b"".join(out)


def _decode_video_planes(stream):
    from cool_chic_amd._lib import Video, check, lib

    v = Video()
    check(lib().ccd_decode_video(stream, len(stream), 0, C.byref(v)), "ccd_decode_video")
    try:
        out = []
        for i in range(v.n_frames):
            f = v.frames[i]
            shapes = [(f.h, f.w), (f.ch, f.cw), (f.ch, f.cw)]
            out.append([np.ctypeslib.as_array(f.plane[p], shape=shapes[p]).copy() for p in range(3)])
        return out
    finally:
        lib().ccd_video_free(C.byref(v))


def _assert_video_equal(got, want, label):
    assert len(got) == len(want), label
    for i, (g, w) in enumerate(zip(got, want)):
        for p in range(3):
            assert np.array_equal(g[p], w["planes"][p]), f"{label}: frame {i} plane {p}"


@pytest.mark.gpu
@pytest.mark.parametrize("fdt,bitdepth,n_taps", [(0, 16, 6), (2, 12, 14), (1, 10, 12), (1, 9, 8), (2, 16, 2), (0, 10, 4)])
def test_decode_video_formats_and_bit_depths(oracle, monkeypatch, fdt, bitdepth, n_taps):
    """vid5's frames re-labelled with another format, bit depth and warp filter size: ccd_decode_video (I-frame planes above
    8 bits, the u16 reference / output paths, the run-time-sized sinc warp) against oracle.decode_video, bit-exact.  The
    8-tap case runs a second time with the warp coefficients computed ahead of the references (CCD_VIDEO_COEF_MB).  14 is the
    largest filter size a frame header carries (4 bits): 16 is reached through ccd_inter_reconstruct only."""
    stream = _rewrite_vid5(fdt, bitdepth, n_taps)
    want = oracle.decode_video(stream)
    assert [f["bitdepth"] for f in want] == [bitdepth] * 5
    monkeypatch.delenv("CCD_VIDEO_COEF_MB", raising=False)
    _assert_video_equal(_decode_video_planes(stream), want, "in-kernel coefficients")
    if n_taps == 8:
        monkeypatch.setenv("CCD_VIDEO_COEF_MB", "4096")
        _assert_video_equal(_decode_video_planes(stream), want, "coefficients ahead")


def crafted_motion_streams(oracle):
    """{name: (stream, flows of the crafted motion cool-chic)}: vid5 with its P frame's motion cool-chic edited the way
    tests/float_classes.py edits networks - what a corrupt or hostile motion network can produce.  The trained motion network
    is all zeros (no motion), so the edits set weights instead of scaling them: synthesis weights +-2^20 and biases
    +-(2^31 - 1) at q step 2^0 give finite flows beyond +-2^31 everywhere ("huge"); upsampling filters of +-2^12 / +-2^16 on top
    make the pyramid overflow: flows that are finite, far or +-inf ("inf"), and mostly NaN ("nan")."""
    from cool_chic_amd import writer

    bs, z, _ = load_golden("vid5")
    _, frames = oracle.split_stream(bs)
    f = next(i for i, (fh, _) in enumerate(frames) if fh.frame_type == 1)
    cc_idx = sum(len(ccs) for _, ccs in frames[:f]) + 1
    hdr, _nn, _lat = frames[f][1][1]
    donor = writer.parse_cc_header(hdr)
    lay = writer.network_layout(donor)
    ints = np.asarray(z[f"cc{cc_idx}.nn_ints"], dtype=np.int64)
    latents = [z[f"cc{cc_idx}.latent{g}"] for g in range(donor.n_grids)]
    q = list(donor.nn_q_step_log2)
    q[4] = q[6] = q[7] = 0  # arm.w arm.b ifce.w ifce.b ups.w ups.b syn.w syn.b (log2)
    arch = writer.derive_arch(donor, nn_q_step_log2=tuple(q))

    def alt(n, v):
        return np.where(np.arange(n) % 3 == 1, -v, v)

    def make(ups_gain, syn_gain, bias):
        g = [x.copy() for x in np.split(ints, np.cumsum(lay)[:-1])]
        if ups_gain:
            g[4] = alt(g[4].size, ups_gain)
        g[6], g[7] = alt(g[6].size, syn_gain), alt(g[7].size, bias)
        cc = writer.encode_coolchic(arch, writer.encode_network(arch, np.concatenate(g).astype(np.int32)), latents)
        stream = _rewrite_vid5(1, 8, 8, motion_edit=(f, cc))
        return stream, oracle.decode_coolchic(*oracle.split_stream(stream)[1][f][1][1])["out"][:2]

    return {"huge": make(0, 2 ** 20, 2 ** 31 - 1), "inf": make(2 ** 12, 2 ** 10, 2 ** 20), "nan": make(2 ** 16, 2 ** 10, 2 ** 20)}


def _check_crafted_flows(streams):
    huge, inf, nan = (streams[k][1] for k in ("huge", "inf", "nan"))
    assert np.isfinite(huge).all() and (np.abs(huge) > 2.0 ** 31).all()
    assert np.isinf(inf).any() and (np.abs(inf[np.isfinite(inf)]) > 2.0 ** 31).any() and not np.isnan(inf).any()
    assert np.isnan(nan).any() and np.isinf(nan).any()


@pytest.mark.gpu
def test_decode_video_crafted_motion(oracle, monkeypatch):
    """A P frame whose motion cool-chic outputs flows beyond +-2^31 and +-inf / NaN: ccd_decode_video with the coefficients in the
    kernel and computed ahead (CCD_VIDEO_COEF_MB), against the oracle, bit-exact - every frame, the B frames that predict from
    the crafted P frame included."""
    streams = crafted_motion_streams(oracle)
    _check_crafted_flows(streams)
    for name, (stream, _) in streams.items():
        want = oracle.decode_video(stream)
        for mb in (None, "4096"):
            if mb is None:
                monkeypatch.delenv("CCD_VIDEO_COEF_MB", raising=False)
            else:
                monkeypatch.setenv("CCD_VIDEO_COEF_MB", mb)
            _assert_video_equal(_decode_video_planes(stream), want, f"{name} CCD_VIDEO_COEF_MB={mb}")


def test_crafted_motion_flows(oracle):
    """The crafted motion cool-chics of the GPU test reach the flows they were built for, and the oracle decodes their
    streams (CPU: oracle only)."""
    streams = crafted_motion_streams(oracle)
    _check_crafted_flows(streams)
    for stream, _ in streams.values():
        assert len(oracle.decode_video(stream)) == 5
