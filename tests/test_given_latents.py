"""Frames synthesised from GIVEN latents (ccd_batch_add_latents, DecodeBatch.add_latents*, RdEvaluator).

The yardstick throughout is the library's own coded path (DecodeBatch.add of range-coded bytes) and its host writer
(writer.encode_coolchic), both pinned by other test files: a given slot must produce the bits the coded slot holding the same
latents produces.  Everything is compared as integer views, without a tolerance.  Nothing here compares the new entry with
itself."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

ERR_VALUE, ERR_ARG = -2, -7
IMAGES = ["odd18x65", "odd100x37", "odd191x127", "rgb192", "cr192", "bicubic190", "bilinear190", "yuv420_8b", "yuv444_10b"]
ALL_MODES = ["rgb192", "cr192", "odd18x65"]  # also run with CCD_OPT_FUSED_DEC = 0 and 1
SAME_FLOAT_KERNELS = 2 | 4 | 64 | 128       # ccd_batch_slot_kernels bits 1, 2, 6, 7


# ---- CPU -------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound():
    from cool_chic_amd import _lib

    with open(os.path.join(ROOT, "include", "ccd.h")) as f:
        header = f.read()
    assert "int ccd_batch_add_latents(ccd_batch* b, const ccd_cc_header* arch, const uint8_t* bytes_nn, size_t n_nn," in header
    assert "ccd_batch_add_latents" in _lib.SIGNATURES
    assert getattr(_lib.lib(), "ccd_batch_add_latents") is not None
    from cool_chic_amd import DecodeBatch

    assert all(hasattr(DecodeBatch, m) for m in ("add_latents", "add_latents_device", "add_latents_from"))
    import cool_chic_amd

    assert cool_chic_amd.RdEvaluator.__name__ == "RdEvaluator"


def test_null_arguments_are_argument_errors_without_a_device():
    from cool_chic_amd._lib import CCHeader, lib

    L = lib()
    arch = CCHeader()
    nn = b"\x00"
    grid = np.zeros(4, np.int8)
    ptrs = (C.c_void_p * 1)(grid.ctypes.data)
    handle = C.create_string_buffer(64)  # stands for a batch: the call must return before it looks at it
    b = C.cast(handle, C.c_void_p)
    for on_device in (0, 1):
        assert L.ccd_batch_add_latents(None, C.byref(arch), nn, 1, ptrs, on_device, 0, 0) == ERR_ARG
        assert L.ccd_batch_add_latents(b, None, nn, 1, ptrs, on_device, 0, 0) == ERR_ARG
        assert L.ccd_batch_add_latents(b, C.byref(arch), None, 0, ptrs, on_device, 0, 0) == ERR_ARG
        assert L.ccd_batch_add_latents(b, C.byref(arch), nn, 1, None, on_device, 0, 0) == ERR_ARG
    assert bytes(handle) == bytes(64)


def test_cli_is_unchanged():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "cc_decode.py"), "--help"], capture_output=True, text=True, timeout=300)
    import re

    assert r.returncode == 0
    assert set(re.findall(r"--[a-z][a-z-]*", r.stdout)) == {"--help", "--input", "--output", "--verbosity", "--device", "--png-level",
                                                           "--source", "--results", "--rate-breakdown", "--no-ms-ssim"}
    import inspect

    from cool_chic_amd.bitstream.decode import decode_video

    assert not any("latent" in p for p in inspect.signature(decode_video).parameters)


# ---- GPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cool_chic_amd import DecodeBatch, _lib

    _lib.lib()
    return DecodeBatch


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _results(batch, slot, bitdepth):
    """Everything a slot produced, on the host: float output, integer planes, the dense stack where the unfused path made one."""
    kernels = batch.slot_kernels(slot)
    return {"output": batch.output(slot), "planes": batch.planes(slot) if bitdepth else [],
            "dense": batch.dense(slot) if not kernels & 4 else None, "kernels": kernels}


def _assert_same_results(got, want, what):
    assert _same(got["output"], want["output"]), (what, "output")
    assert len(got["planes"]) == len(want["planes"]), what
    for p, (a, b) in enumerate(zip(got["planes"], want["planes"])):
        assert _same(a, b), (what, "plane", p)
    assert (got["dense"] is None) == (want["dense"] is None), what
    if want["dense"] is not None:
        assert _same(got["dense"], want["dense"]), (what, "dense")


def _cool_chics(oracle, name):
    """[(triple, bitdepth, frame_data_type)] of a fixture; the cool-chics of a video are taken with bitdepth 0 (float output only)."""
    _, frames = oracle.split_stream(load_golden(name)[0])
    if name.startswith("vid"):
        return [(cc, 0, fh.frame_data_type) for fh, ccs in frames for cc in ccs]
    (fh, ccs), = frames
    return [(ccs[0], fh.bitdepth, fh.frame_data_type)]


_CODED = {}


def _coded(gpu, oracle, name, mode=None):
    """The fixture through the coded path, once per (name, mode): {"jobs": [(arch, nn, latents, bitdepth, fdt)], "res": [results],
    "batch": the decoded batch, kept for its device latents}."""
    key = (name, mode)
    if key not in _CODED:
        b = gpu(0, fused_dec=mode)
        ccs = _cool_chics(oracle, name)
        for (hdr, nn, lat), bd, fdt in ccs:
            b.add(hdr, nn, lat, bd, fdt)
        b.run(); b.wait()
        jobs, res = [], []
        for s, ((hdr, nn, lat), bd, fdt) in enumerate(ccs):
            h = b.header(s)
            jobs.append((h, nn, [b.latent(s, g) for g in range(h.n_grids)], bd, fdt))
            res.append(_results(b, s, bd))
        _CODED[key] = {"jobs": jobs, "res": res, "batch": b}
    return _CODED[key]


def _check_given_batch(batch, want, what):
    """Tests 1 and 2 for a batch made only of given slots that has run."""
    from cool_chic_amd._lib import lib

    assert lib().ccd_batch_wait(batch._h, None) == 0, what
    assert batch.entropy_launches() == 0, what
    for s, w in enumerate(want):
        assert batch.slot_status(s) == 0, (what, s)
        assert not batch.slot_stats(s)[1:4].any(), (what, s)
        got = _results(batch, s, len(w["planes"]) and 8)
        k = got["kernels"]
        assert k & 256 and not k & 1 and not k & (8 | 16 | 32), (what, s, k)
        assert k & SAME_FLOAT_KERNELS == w["kernels"] & SAME_FLOAT_KERNELS, (what, s, k, w["kernels"])
        _assert_same_results(got, w, (what, s))


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", [(n, None) for n in IMAGES + ["vid3_ldp"]] + [(n, m) for n in ALL_MODES for m in (0, 1, 2)])
def test_bit_equality_with_the_coded_path(gpu, oracle, name, mode):
    ref = _coded(gpu, oracle, name, mode)
    assert len(ref["jobs"]) == (5 if name == "vid3_ldp" else 1)
    host, dev = gpu(0, fused_dec=mode), gpu(0, fused_dec=mode)
    for s, (arch, nn, lat, bd, fdt) in enumerate(ref["jobs"]):
        assert host.add_latents(arch, nn, lat, bd, fdt) == s
        assert dev.add_latents_from(ref["batch"], s, bitdepth=bd, frame_data_type=fdt) == s
    for b, what in ((host, "host"), (dev, "device")):
        b.run(); b.wait()
        _check_given_batch(b, ref["res"], (name, mode, what))
        for s, (arch, _, lat, _, _) in enumerate(ref["jobs"]):  # the grids sit where ccd_batch_latent says
            assert all(np.array_equal(b.latent(s, g), lat[g]) for g in range(arch.n_grids)), (name, what, s)
        b.close()


_RANDOM = {}


def _random_case(gpu, oracle, name):
    """Latents the fixture's stream never held - the whole alphabet from a seeded generator, one grid of -64, one of 63, one of
    zeros - encoded by the HOST writer and decoded through the coded path: (arch, nn, latents, bitdepth, fdt, results)."""
    if name not in _RANDOM:
        from cool_chic_amd import writer

        arch, nn, lat0, bd, fdt = _coded(gpu, oracle, name)["jobs"][0]
        rng = np.random.default_rng(len(name))
        lat = [rng.integers(-64, 64, size=a.shape, dtype=np.int8) for a in lat0]
        assert len(lat) >= 4 and min(int(a.min()) for a in lat) == -64 and max(int(a.max()) for a in lat) == 63
        lat[1][:], lat[2][:], lat[3][:] = -64, 63, 0
        cc = writer.encode_coolchic(arch, nn, lat)
        h2 = writer.parse_cc_header(cc)
        p, q = h2.n_bytes_header, h2.n_bytes_header + h2.nn_n_bytes
        b = gpu(0)
        b.add(cc[:p], cc[p:q], cc[q:], bd, fdt)
        b.run(); b.wait()
        assert all(np.array_equal(b.latent(0, g), lat[g]) for g in range(len(lat)))
        _RANDOM[name] = (arch, nn, lat, bd, fdt, _results(b, 0, bd))
        b.close()
    return _RANDOM[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rgb192", "odd18x65"])
def test_latents_the_stream_never_held(gpu, oracle, name):
    arch, nn, lat, bd, fdt, want = _random_case(gpu, oracle, name)
    b = gpu(0)
    b.add_latents(arch, nn, lat, bd, fdt)
    b.run(); b.wait()
    _check_given_batch(b, [want], name)
    assert not _same(want["planes"][0], _coded(gpu, oracle, name)["res"][0]["planes"][0])  # and they are other planes than the fixture's
    b.close()


MIXED = [("rgb192", False), ("cr192", True), ("odd18x65", False), ("odd100x37", True), ("yuv420_8b", False), ("yuv444_10b", True)]


@pytest.mark.gpu
@pytest.mark.parametrize("overlap", [0, 1])
def test_mixed_batch_and_determinism(gpu, oracle, overlap):
    """Three coded and three given slots, interleaved: every slot gives what it gives alone, the entropy launches are those of
    the three coded slots, and a second run gives the same bytes."""
    refs = [_coded(gpu, oracle, name) for name, _ in MIXED]
    only_coded, mixed = gpu(0, overlap=bool(overlap)), gpu(0, overlap=bool(overlap))
    for (name, given), ref in zip(MIXED, refs):
        arch, nn, lat, bd, fdt = ref["jobs"][0]
        (hdr, nn0, payload), _, _ = _cool_chics(oracle, name)[0]
        if given:
            if name == "odd100x37":
                mixed.add_latents_from(ref["batch"], 0, bitdepth=bd, frame_data_type=fdt)
            else:
                mixed.add_latents(arch, nn, lat, bd, fdt)
        else:
            mixed.add(hdr, nn0, payload, bd, fdt)
            only_coded.add(hdr, nn0, payload, bd, fdt)
    only_coded.run(); only_coded.wait()
    runs = []
    for _ in range(2):
        mixed.run(); mixed.wait()
        runs.append([_results(mixed, s, refs[s]["jobs"][0][3]) for s in range(len(MIXED))])
    assert mixed.entropy_launches() == only_coded.entropy_launches() >= 1
    for s, ((name, given), ref) in enumerate(zip(MIXED, refs)):
        assert bool(mixed.slot_kernels(s) & 256) == given and mixed.slot_status(s) == 0
        _assert_same_results(runs[0][s], ref["res"][0], (name, "mixed"))
        _assert_same_results(runs[1][s], runs[0][s], (name, "second run"))
        if given:
            assert not mixed.slot_stats(s)[1:4].any()
        else:
            assert mixed.slot_stats(s)[1] > 0
    # a given slot alone, against the same slot inside the mixed batch
    arch, nn, lat, bd, fdt = refs[1]["jobs"][0]
    alone = gpu(0, overlap=bool(overlap))
    alone.add_latents(arch, nn, lat, bd, fdt)
    alone.run(); alone.wait()
    _assert_same_results(_results(alone, 0, bd), runs[0][1], "cr192 alone")
    for b in (alone, mixed, only_coded):
        b.close()


def _device_buffer(latents, offsets=None, pad=64, sentinel=0x55):
    """One int8 CUDA buffer that holds every grid with `pad` sentinel bytes (a value OUTSIDE the alphabet) around it, grid g at
    a 256-byte boundary + offsets[g]; returns (tensor, [byte position of grid g])."""
    import torch

    pos, at = [], 0
    for g, a in enumerate(latents):
        at = (at + pad + 255) // 256 * 256 + (offsets[g % len(offsets)] if offsets else 0)
        pos.append(at)
        at += a.size
    host = np.full(at + pad, sentinel, np.uint8)
    for p, a in zip(pos, latents):
        host[p:p + a.size] = a.astype(np.int8).view(np.uint8).ravel()
    return torch.from_numpy(host.view(np.int8)).cuda(), pos


def _fill(buf, pos, latents):
    import torch

    for p, a in zip(pos, latents):
        buf[p:p + a.size] = torch.from_numpy(np.ascontiguousarray(a, np.int8).ravel()).cuda()
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_device_latents_are_read_at_every_run(gpu, oracle):
    ref = _coded(gpu, oracle, "rgb192")
    arch, nn, lat, bd, fdt = ref["jobs"][0]
    _, _, lat2, _, _, want2 = _random_case(gpu, oracle, "rgb192")
    buf, pos = _device_buffer(lat)
    b = gpu(0)
    b.add_latents_device(arch, nn, [buf.data_ptr() + p for p in pos], bd, fdt, owner=buf)
    b.run(); b.wait()
    _check_given_batch(b, ref["res"], "first run")
    _fill(buf, pos, lat2)
    b.run(); b.wait()
    _check_given_batch(b, [want2], "after the latents changed in place")
    b.close()


@pytest.mark.gpu
def test_alphabet(gpu, oracle):
    from cool_chic_amd._lib import CcdError

    ref = _coded(gpu, oracle, "rgb192")
    arch, nn, lat, bd, fdt = ref["jobs"][0]
    # host latents: refused at add, no slot
    b = gpu(0)
    b.add_latents(arch, nn, lat, bd, fdt)
    for grid, value in ((0, 64), (arch.n_grids - 1, -65), (2, 127), (1, -128)):
        bad = [a.copy() for a in lat]
        bad[grid].flat[bad[grid].size // 2] = value
        with pytest.raises(CcdError) as e:
            b.add_latents(arch, nn, bad, bd, fdt)
        assert e.value.code == ERR_VALUE and len(b) == 1
    b.close()
    # device latents: that slot's status at wait, the other slots untouched, and OK again once the buffer is repaired
    for grid, value in ((0, 64), (arch.n_grids - 1, -65)):
        bad = [a.copy() for a in lat]
        bad[grid].flat[bad[grid].size - 1] = value
        good_buf, good_pos = _device_buffer(lat)
        bad_buf, bad_pos = _device_buffer(bad)
        b = gpu(0)
        b.add_latents_device(arch, nn, [good_buf.data_ptr() + p for p in good_pos], bd, fdt, owner=good_buf)
        b.add_latents_device(arch, nn, [bad_buf.data_ptr() + p for p in bad_pos], bd, fdt, owner=bad_buf)
        b.add_latents(arch, nn, lat, bd, fdt)
        b.run()
        with pytest.raises(CcdError) as e:
            b.wait()
        assert e.value.code == ERR_VALUE
        assert [b.slot_status(s) for s in range(3)] == [0, ERR_VALUE, 0]
        for s in (0, 2):
            _assert_same_results(_results(b, s, bd), ref["res"][0], ("beside a refused slot", s))
        b.run()  # the same latents again: still that slot's error, not a stale or a lost one
        with pytest.raises(CcdError):
            b.wait()
        assert [b.slot_status(s) for s in range(3)] == [0, ERR_VALUE, 0]
        _fill(bad_buf, bad_pos, lat)
        for _ in range(2):
            b.run(); b.wait()
            assert [b.slot_status(s) for s in range(3)] == [0, 0, 0]
            _check_given_batch(b, ref["res"] * 3, "repaired")
        b.close()


@pytest.mark.gpu
def test_ragged_copies(gpu, oracle):
    """Source grids at byte offsets 1, 3 and 7 (w x h: 18 x 65, 3 x 9, 5 x 17 and, the smallest this pyramid has, 1 x 3 and 1 x 2),
    sentinels outside the alphabet around each: the planes of the aligned case, no error from a byte beside a grid, and the
    buffer unchanged."""
    ref = _coded(gpu, oracle, "odd18x65")
    arch, nn, lat, bd, fdt = ref["jobs"][0]
    assert {(2, 1), (3, 1), (9, 3), (17, 5), (65, 18)} <= {a.shape for a in lat}  # (h, w)
    b = gpu(0)
    bufs = []
    for offsets in ([1, 3, 7], [7, 1, 3], [3, 7, 1], [16, 32, 48]):
        buf, pos = _device_buffer(lat, offsets)
        assert offsets[0] == 16 or any(p % 16 in (1, 3, 7) for p in pos)
        b.add_latents_device(arch, nn, [buf.data_ptr() + p for p in pos], bd, fdt, owner=buf)
        bufs.append((buf, buf.cpu().numpy().copy()))
    b.run(); b.wait()
    _check_given_batch(b, ref["res"] * len(bufs), "ragged")
    for buf, before in bufs:
        assert np.array_equal(buf.cpu().numpy(), before)
    b.close()


def _perturbed_networks(arch, nn_ints, want=3, seed=0):
    """`want` networks whose ARM weights differ from nn_ints by +-1 in six places and that writer.encode_network accepts
    (the perturbation of test_device_rate.py::test_candidates_that_share_latents, restated): [(arch with its own nn_n_bytes,
    payload)].  A change of the ARM alone would leave the planes as they are, so two synthesis weights move as well."""
    from cool_chic_amd import writer
    from cool_chic_amd._lib import CCHeader

    rng = np.random.default_rng(seed)
    layout = writer.network_layout(arch)
    n_arm_w, syn_first = layout[0], sum(layout[:6])
    out = []
    for _ in range(4 * want):
        values = np.array(nn_ints, np.int64)
        where = rng.choice(n_arm_w, size=6, replace=False)
        values[where] += rng.choice([-1, 1], size=6)
        where = syn_first + rng.choice(layout[6], size=2, replace=False)
        values[where] += rng.choice([-1, 1], size=2)
        a = CCHeader.from_buffer_copy(bytes(arch))
        try:
            nn = writer.encode_network(a, values)
        except Exception:  # noqa: BLE001  (a value the Exp-Golomb orders of the header cannot carry)
            continue
        out.append((a, nn))
        if len(out) == want:
            break
    return out


@pytest.fixture(scope="module")
def candidates(gpu, oracle):
    """rgb192 and three perturbed networks over ITS latents, each through the host writer and the coded path:
    [(arch, nn, results of the coded path)], the latents, the decoded rgb192 batch."""
    from cool_chic_amd import writer

    ref = _coded(gpu, oracle, "rgb192")
    arch, nn, lat, bd, fdt = ref["jobs"][0]
    (hdr, nn0, payload), _, _ = _cool_chics(oracle, "rgb192")[0]
    nn_ints = oracle.decode_coolchic(hdr, nn0, payload, stop_after_entropy=True)["nn_ints"]
    out = [(arch, nn, ref["res"][0])]
    coded = gpu(0)
    for a, nn_k in _perturbed_networks(arch, nn_ints):
        cc = writer.encode_coolchic(a, nn_k, lat)
        h2 = writer.parse_cc_header(cc)
        p, q = h2.n_bytes_header, h2.n_bytes_header + h2.nn_n_bytes
        assert cc[p:q] == nn_k
        s = coded.add(cc[:p], cc[p:q], cc[q:], bd, fdt)
        out.append((h2, nn_k, s))
    assert len(out) == 4
    coded.run(); coded.wait()
    out = [out[0]] + [(a, n, _results(coded, s, bd)) for a, n, s in out[1:]]
    yield out, lat, ref["batch"], coded
    coded.close()


@pytest.mark.gpu
def test_candidates_that_share_latents(gpu, candidates):
    cands, lat, decoded, coded = candidates
    b = gpu(0)
    for a, nn_k, _ in cands:
        b.add_latents_from(decoded, 0, arch=a, bytes_nn=nn_k, bitdepth=8, frame_data_type=0)
    b.run(); b.wait()
    _check_given_batch(b, [w for _, _, w in cands], "candidates")
    for s in range(1, 4):  # the coded slots did decode these latents
        assert all(np.array_equal(coded.latent(s - 1, g), lat[g]) for g in range(len(lat)))
    distinct = {b"".join(p.tobytes() for p in w["planes"]) for _, _, w in cands}
    assert len(distinct) >= 2
    b.close()


@pytest.mark.gpu
def test_rd_evaluator(gpu, candidates):
    import torch

    from cool_chic_amd import EncodeBatch, RdEvaluator
    from cool_chic_amd._lib import lib
    from cool_chic_amd.quality import QualityMeter, _planes_to_frame_data

    cands, lat, decoded, coded = candidates
    source = _planes_to_frame_data(cands[0][2]["planes"], 8, "rgb")
    n_pixels = 128 * 192
    assert source.n_pixels == n_pixels
    ptrs = [lib().ccd_batch_latent(decoded._h, 0, g) for g in range(len(lat))]
    ev = RdEvaluator(0)
    for k, (a, nn_k, _) in enumerate(cands):  # host latents and device latents side by side
        ev.add(a, nn_k, lat if k % 2 == 0 else ptrs, source, owner=decoded)
    # the yardsticks: the rate meter on the same candidates, the quality meter on the coded path's planes
    enc = EncodeBatch(0)
    for a, nn_k, _ in cands:
        enc.add(a, nn_k, lat)
    enc.measure(); enc.wait()
    rates = [enc.rate(s) for s in range(4)]
    src_planes = [torch.from_numpy(p).cuda() for p in cands[0][2]["planes"]]
    dec_planes = [[torch.from_numpy(p).cuda() for p in w["planes"]] for _, _, w in cands]
    bits64 = lambda r: np.concatenate([r.bits, [r.total_bits]]).astype(np.float64).view(np.uint64).tolist()  # noqa: E731
    with QualityMeter(0) as meter:
        for ms_ssim in (False, True):
            want_q = meter.score_planes(dec_planes, [src_planes] * 4, [8] * 4, ["rgb"] * 4, ms_ssim)
            best = {}
            for lmbda in (0.0, 1e-3, 1.0):
                got = ev.evaluate(lmbda, ms_ssim=ms_ssim)
                assert len(got) == 4
                for k, (c, r, q) in enumerate(zip(got, rates, want_q)):
                    assert c.rate.status == 0 and bits64(c.rate) == bits64(r), k
                    assert c.rate.sum_width.tolist() == r.sum_width.tolist() and c.rate.n_symbols.tolist() == r.n_symbols.tolist()
                    assert (c.rate.n_bytes_nn, c.rate.n_bytes_header) == (r.n_bytes_nn, r.n_bytes_header) == (len(cands[k][1]), r.n_bytes_header)
                    for f in ("bitdepth", "frame_data_type", "sse", "n", "n_scales", "cs", "ssim"):
                        assert getattr(c.quality, f) == getattr(q, f), (k, f)
                    assert repr(c.quality.psnr_db) == repr(q.psnr_db) and repr(c.quality.ms_ssim) == repr(q.ms_ssim)
                    # the float64 formula, from the device's integers
                    mse = float(sum(q.sse)) / (float(sum(q.n)) * 255.0 * 255.0)
                    bits = float(r.total_bits) + 8.0 * float(r.n_bytes_nn + r.n_bytes_header)
                    assert c.mse == mse and c.bits == bits and c.cost == mse + float(lmbda) * bits / float(n_pixels), k
                    print(f"lambda {lmbda} candidate {k}: sse {sum(q.sse)} bits {bits:.3f} cost {c.cost:.9g}")
                assert sum(got[0].quality.sse) == 0 and got[0].cost == lmbda * got[0].bits / n_pixels
                assert sum(q.n) == 3 * n_pixels
                assert any(sum(c.quality.sse) > 0 for c in got[1:])
                costs = [c.cost for c in got]
                want_costs = [float(sum(q.sse)) / (float(sum(q.n)) * 65025.0) + lmbda * (r.total_bits + 8.0 * (r.n_bytes_nn + r.n_bytes_header)) / n_pixels
                              for q, r in zip(want_q, rates)]
                best[lmbda] = int(np.argmin(costs))
                assert best[lmbda] == int(np.argmin(want_costs))
            assert best[0.0] == 0
    enc.close()
    ev.close()
