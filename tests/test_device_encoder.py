"""The device writer (ccd_enc_*, cool_chic_amd.encoder.EncodeBatch) against the reference-encoded
fixtures and the host writer.  Everything here is byte equality: there is no tolerance anywhere in this feature."""
import ctypes as C
import threading

import numpy as np
import pytest

from conftest import load_golden

ERR_VALUE, ERR_HIP, ERR_ARG = -2, -6, -7
ENTRY_POINTS = ["ccd_enc_create", "ccd_enc_destroy", "ccd_enc_add", "ccd_enc_size", "ccd_enc_run", "ccd_enc_wait",
                "ccd_enc_slot_bytes", "ccd_enc_slot_payload", "ccd_enc_slot_status", "ccd_enc_payload_bound"]


def _cool_chics(oracle, bs):
    """[(cool-chic header, NN payload, latent payload)] of every cool-chic of a stream, coding order."""
    _, frames = oracle.split_stream(bs)
    return [cc for _, ccs in frames for cc in ccs]


def _fixture_latents(z, arch, i):
    return [z[f"cc{i}.latent{g}"] for g in range(arch.n_grids)]


def _split_cc(cc: bytes):
    from cool_chic_amd import writer

    h = writer.parse_cc_header(cc)
    a, b = h.n_bytes_header, h.n_bytes_header + h.nn_n_bytes
    assert len(cc) == b + h.n_bytes_latent
    return cc[:a], cc[a:b], cc[b:]


# ---- CPU -------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_exported():
    import os

    from cool_chic_amd import EncodeBatch, _lib, encoder  # noqa: F401

    with open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "ccd.h")) as f:
        header = f.read()
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert name + "(" in header, name
        assert name in _lib.SIGNATURES, name
        assert getattr(L, name) is not None


def test_null_handles_are_argument_errors():
    from cool_chic_amd._lib import CCHeader, lib

    L = lib()
    assert L.ccd_enc_create(0, None) == ERR_ARG
    h = CCHeader()
    ptrs = (C.c_void_p * 1)(None)
    out = C.POINTER(C.c_uint8)()
    dev = C.c_void_p()
    assert L.ccd_enc_add(None, C.byref(h), b"x", 1, ptrs, 0) == ERR_ARG
    assert L.ccd_enc_size(None) == ERR_ARG
    assert L.ccd_enc_run(None, None) == ERR_ARG
    assert L.ccd_enc_wait(None, None) == ERR_ARG
    assert L.ccd_enc_slot_bytes(None, 0, C.byref(out)) == ERR_ARG and not out
    assert L.ccd_enc_slot_payload(None, 0, C.byref(dev)) == ERR_ARG and not dev.value
    assert L.ccd_enc_slot_status(None, 0, None) == ERR_ARG
    L.ccd_enc_destroy(None)  # returns nothing, does nothing


def test_create_reports_a_missing_device():
    """Without a usable GPU ccd_enc_create is CCD_ERR_HIP and leaves *out NULL (with one it succeeds); a device index that
    does not exist is CCD_ERR_HIP everywhere."""
    import torch

    from cool_chic_amd._lib import lib

    h = C.c_void_p(0x1234)
    assert lib().ccd_enc_create(4096, C.byref(h)) == ERR_HIP and not h.value
    h = C.c_void_p(0x1234)
    rc = lib().ccd_enc_create(0, C.byref(h))
    if torch.cuda.is_available():
        assert rc == 0 and h.value
        lib().ccd_enc_destroy(h)
    else:
        assert rc == ERR_HIP and not h.value


def test_payload_bound_holds_for_far_tail_symbols():
    """Every symbol at the far tail of its distribution (mu = -64, symbol 63: an interval of the model's floor, 1 / 2^24
    plus nothing) is the most a symbol can cost; the host coder's output stays inside the bound the device buffers use."""
    from cool_chic_amd import writer
    from cool_chic_amd._lib import lib

    bound = lib().ccd_enc_payload_bound
    assert bound(0) > 0
    assert bound(1000) == 4 * ((24 * 1000 + 31) // 32 + 2)
    for n in (1, 2, 3, 4, 5, 63, 64, 1000, 20001):
        sym = np.full(n, 63, np.int8)
        mu = np.zeros(n, np.int32)
        for sc in (np.zeros(n, np.int32), np.full(n, 2560, np.int32), (np.arange(n) % 2 * 2560).astype(np.int32)):
            assert len(writer.range_encode(sym, mu, sc)) <= bound(n), (n, int(sc[-1]))
        # and the other tail
        assert len(writer.range_encode(np.full(n, -64, np.int8), np.full(n, 32767, np.int32), np.zeros(n, np.int32))) <= bound(n)


def test_host_path_is_unchanged_by_the_device_argument(oracle):
    from cool_chic_amd import writer

    bs, z, _ = load_golden("rgb192")
    hdr, nn, lat = _cool_chics(oracle, bs)[0]
    arch = writer.parse_cc_header(hdr)
    latents = _fixture_latents(z, arch, 0)
    assert writer.encode_coolchic(arch, nn, latents, device=None) == writer.encode_coolchic(arch, nn, latents) == hdr + nn + lat
    assert writer.encode_stream(hdr, nn, latents, device=None) == writer.encode_stream(hdr, nn, latents) == bs


# ---- GPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cool_chic_amd import EncodeBatch, _lib

    _lib.lib()
    return EncodeBatch


def _check_bound(enc, slot, arch):
    from cool_chic_amd.encoder import payload_bound

    n = enc.payload(slot).__cuda_array_interface__["shape"][0]
    assert n <= payload_bound(arch.n_symbols), (slot, n)
    return n


def _encode_all(gpu, jobs):
    """jobs = [(arch, nn, latents)] -> device bytes per job, one handle, one run."""
    enc = gpu(0)
    try:
        for arch, nn, latents in jobs:
            enc.add(arch, nn, latents)
        enc.run()
        enc.wait()
        out = []
        for i, (arch, _, _) in enumerate(jobs):
            out.append(enc.bytes(i))
            n_lat = _check_bound(enc, i, arch)
            assert out[-1][len(out[-1]) - n_lat:] == bytes(_device_bytes(enc.payload(i)))
        return out
    finally:
        enc.close()


def _device_bytes(dev_array):
    import torch

    if dev_array.__cuda_array_interface__["shape"][0] == 0:
        return b""
    return torch.as_tensor(dev_array, device="cuda").cpu().numpy().tobytes()


@pytest.mark.gpu
def test_reference_fixtures_byte_for_byte(gpu, oracle):
    """Reference-decoded latents of every cool-chic of the reference-ENCODED fixtures -> the cool-chic's bytes in the file."""
    from cool_chic_amd import writer

    jobs, want = [], []
    for name in ["kodim14", "rgb192", "yuv420_8b", "yuv420_10b", "yuv444_10b", "vid5"]:
        bs, z, _ = load_golden(name)
        for i, (hdr, nn, lat) in enumerate(_cool_chics(oracle, bs)):
            arch = writer.parse_cc_header(hdr)
            jobs.append((arch, nn, _fixture_latents(z, arch, i)))
            want.append((name, i, hdr + nn + lat))
    got = _encode_all(gpu, jobs)
    for (name, i, w), g in zip(want, got):
        assert g == w, (name, i)
    # the coder's carry path is exercised by these inputs, both ways (counts of the host coder: DESIGN.md 4.10)
    enc = gpu(0)
    enc.add(*jobs[0])
    enc.run()
    enc.wait()
    status, counters = enc.slot_status(0)
    print("kodim14: words %d, inverted runs %d, resolved with carry %d, without %d" % tuple(counters[1:5]))
    assert status == 0 and counters[1] == 7738 and tuple(counters[2:5]) == (3909, 1925, 1984)
    enc.close()


def _extreme_latents(arch, seed=5):
    """Symbols -64 and 63 next to each other (checkerboard patches) inside otherwise Laplacian grids."""
    rng = np.random.default_rng(seed)
    out = []
    for g in range(arch.n_grids):
        h, w = arch.grid_h[g], arch.grid_w[g]
        a = np.clip(np.round(rng.laplace(size=(h, w)) * 3), -64, 63).astype(np.int8)
        yy, xx = np.mgrid[0:h, 0:w]
        patch = ((yy // 7 + xx // 5) % 3 == 0)
        a[patch] = np.where((yy + xx) % 2 == 0, -64, 63).astype(np.int8)[patch]
        out.append(a)
    return out


@pytest.mark.gpu
def test_host_writer_is_the_yardstick(gpu, oracle):
    from cool_chic_amd import DecodeBatch, synth, writer

    jobs, names = [], []
    for name in ["hq192", "cr192", "mop192", "vhop192", "bicubic190", "odd18x65", "odd100x37", "odd191x127"]:
        bs, z, _ = load_golden(name)
        hdr, nn, _ = _cool_chics(oracle, bs)[0]
        arch = writer.parse_cc_header(hdr)
        jobs.append((arch, nn, _fixture_latents(z, arch, 0)))
        names.append(name)
    bs, z, _ = load_golden("rgb192")
    hdr, nn, _ = _cool_chics(oracle, bs)[0]
    arch = writer.parse_cc_header(hdr)
    lat = _fixture_latents(z, arch, 0)
    _, levels = writer.grid_sizes((arch.img_size[0], arch.img_size[1]), hdr)
    jobs.append((arch, nn, writer.variant_latents(lat, levels, 11, False))); names.append("rgb192 rolled")
    t_arch = writer.derive_arch(arch, img_size=(arch.img_size[1], arch.img_size[0]))
    jobs.append((t_arch, nn, writer.variant_latents(lat, levels, 12, True))); names.append("rgb192 transposed")
    jobs.append((arch, nn, _extreme_latents(arch))); names.append("rgb192 extremes")
    # weights and worst-case features beyond 16- / 32-bit operands; the latents are what the (separately verified) decoder
    # reads out of the streams the benchmark uses
    wide, _ = synth.kodak24_wide_envelope()
    picked = [_cool_chics(oracle, wide[k])[0] for k in (0, 3, 17)]
    dec = DecodeBatch(0)
    for w_hdr, w_nn, w_lat in picked:
        dec.add(w_hdr, w_nn, w_lat, 0, 0)
    dec.run(); dec.wait()
    for k, (w_hdr, w_nn, _) in enumerate(picked):
        w_arch = writer.parse_cc_header(w_hdr)
        jobs.append((w_arch, w_nn, [dec.latent(k, g) for g in range(w_arch.n_grids)])); names.append(f"wide envelope {k}")
    dec.close()
    got = _encode_all(gpu, jobs)
    for name, (a, nn_, lat_), g in zip(names, jobs, got):
        assert g == writer.encode_coolchic(a, nn_, lat_), name
    for k in range(3):
        assert got[len(jobs) - 3 + k] == b"".join(picked[k]), k
    # the convenience wrappers frame the same bytes
    a, nn_, lat_ = jobs[0]
    assert writer.encode_coolchic(a, nn_, lat_, device=0) == got[0]
    bs, _, _ = load_golden("rgb192")
    assert writer.encode_stream(hdr, nn, lat, device=0) == bs


@pytest.mark.gpu
def test_grids_on_the_edges_of_the_coding_order(gpu, oracle, monkeypatch):
    """Pictures whose grids sit where the coding order (ccd_wavefront.hpp) changes its rule: widths 9 / 10 / 11 (raster against
    wavefront) and 18 .. 21, 36 .. 42 (a step's first column moving into the next ten).  kodim14's networks, seeded random
    latents: the device writer's bytes are the host writer's, and both entropy kernels read the same latents back."""
    from cool_chic_amd import DecodeBatch, writer

    bs, z, _ = load_golden("kodim14")
    hdr, nn, _ = _cool_chics(oracle, bs)[0]
    donor = writer.parse_cc_header(hdr)
    rng = np.random.default_rng(20241019)
    jobs = []
    for size, widths in [((12, 40), (40, 20, 10, 5)), ((11, 42), (42, 21, 11, 6)), ((7, 36), (36, 18, 9)), ((3, 19), (19, 10, 5))]:
        arch = writer.derive_arch(donor, img_size=size)
        assert tuple(arch.grid_w[:len(widths)]) == widths
        nn_i = nn
        if writer.network_layout(arch) != writer.network_layout(donor):  # (3 rows: a grid's level comes from the height ratio)
            nn_i = writer.encode_network(arch, writer.adapt_network(donor, z["cc0.nn_ints"], arch))
        lat = [np.clip(np.rint(rng.laplace(0.0, 1.5, size=(arch.grid_h[g], arch.grid_w[g]))), -30, 30).astype(np.int8)
               for g in range(arch.n_grids)]
        jobs.append((arch, nn_i, lat))
    got = _encode_all(gpu, jobs)
    for (arch, nn_i, lat), cc in zip(jobs, got):
        assert cc == writer.encode_coolchic(arch, nn_i, lat), tuple(arch.img_size)
    for generic in (0, 1):
        monkeypatch.setenv("CCD_FORCE_GENERIC", str(generic))  # read when a batch is created
        dec = DecodeBatch(0)
        try:
            for cc in got:
                dec.add(*_split_cc(cc), 8, 0)
            dec.run()
            dec.wait()
            for i, (arch, _, lat) in enumerate(jobs):
                assert dec.slot_status(i) == 0 and (dec.slot_kernels(i) & 1) == 1 - generic, (i, generic)
                for g, a in enumerate(lat):
                    assert np.array_equal(dec.latent(i, g), a), (tuple(arch.img_size), g, generic)
        finally:
            dec.close()


def _round_trip(gpu, oracle, streams):
    """Decode every cool-chic of `streams` in one DecodeBatch, hand all slots to one EncodeBatch without leaving the device,
    compare with the bytes that were decoded; then decode the device-written payloads again: same latents."""
    from cool_chic_amd import DecodeBatch

    ccs = [cc for bs in streams for cc in _cool_chics(oracle, bs)]
    dec = DecodeBatch(0)
    for hdr, nn, lat in ccs:
        dec.add(hdr, nn, lat, 0, 0)
    dec.run()
    dec.wait()
    enc = gpu(0)
    for s in range(len(ccs)):
        assert enc.add_from_decode(dec, s) == s
    enc.run()
    enc.wait()
    got = [enc.bytes(s) for s in range(len(ccs))]
    for s, (hdr, nn, lat) in enumerate(ccs):
        assert got[s] == hdr + nn + lat, s
        _check_bound(enc, s, dec.header(s))
    back = DecodeBatch(0)
    for s in range(len(ccs)):
        h2, n2, l2 = _split_cc(got[s])
        l2_dev = _device_bytes(enc.payload(s))
        assert l2_dev == l2
        back.add(h2, n2, l2_dev, 0, 0)
    back.run()
    back.wait()
    for s in range(len(ccs)):
        for g in range(dec.header(s).n_grids):
            assert np.array_equal(back.latent(s, g), dec.latent(s, g)), (s, g)
    enc.close(); dec.close(); back.close()
    return len(ccs)


@pytest.mark.gpu
def test_round_trip_kodak24_without_the_host(gpu, oracle):
    from cool_chic_amd import synth

    assert _round_trip(gpu, oracle, synth.workload("kodak24")["streams"]) == 24


@pytest.mark.gpu
def test_round_trip_gop1080p(gpu, oracle):
    from cool_chic_amd import synth

    bs, info = synth.gop1080p(2)
    assert _round_trip(gpu, oracle, [bs]) == info["cool_chics"] == 4  # I, I, and two cool-chics for the B frame


@pytest.mark.gpu
def test_round_trip_4k(gpu, oracle):
    from cool_chic_amd import synth

    assert _round_trip(gpu, oracle, [synth.image_stream(2160, 3840)]) == 1


def _rgb192(oracle):
    from cool_chic_amd import writer

    bs, z, _ = load_golden("rgb192")
    hdr, nn, lat = _cool_chics(oracle, bs)[0]
    arch = writer.parse_cc_header(hdr)
    return arch, nn, [np.ascontiguousarray(a, dtype=np.int8) for a in _fixture_latents(z, arch, 0)], hdr + nn + lat


@pytest.mark.gpu
def test_argument_checks_on_a_live_handle(gpu, oracle):
    from cool_chic_amd._lib import CCHeader, lib

    L = lib()
    arch, nn, lat, want = _rgb192(oracle)
    enc = gpu(0)
    h = enc._h
    ptrs = (C.c_void_p * len(lat))(*[a.ctypes.data for a in lat])
    assert L.ccd_enc_add(h, None, nn, len(nn), ptrs, 0) == ERR_ARG
    assert L.ccd_enc_add(h, C.byref(arch), None, len(nn), ptrs, 0) == ERR_ARG
    assert L.ccd_enc_add(h, C.byref(arch), nn, len(nn), None, 0) == ERR_ARG
    holed = (C.c_void_p * len(lat))(*[a.ctypes.data for a in lat])
    holed[1] = None
    assert L.ccd_enc_add(h, C.byref(arch), nn, len(nn), holed, 0) == ERR_ARG
    assert L.ccd_enc_add(h, C.byref(arch), nn, len(nn), holed, 1) == ERR_ARG
    bad = CCHeader.from_buffer_copy(bytes(arch))
    bad.img_size[0] = 0  # does not re-parse
    assert L.ccd_enc_add(h, C.byref(bad), nn, len(nn), ptrs, 0) == ERR_VALUE
    for v in (64, -65):
        poisoned = [a.copy() for a in lat]
        poisoned[2][1, 1] = v
        pp = (C.c_void_p * len(lat))(*[a.ctypes.data for a in poisoned])
        assert L.ccd_enc_add(h, C.byref(arch), nn, len(nn), pp, 0) == ERR_VALUE
    assert len(enc) == 0  # nothing was added or enqueued
    out = C.POINTER(C.c_uint8)()
    dev = C.c_void_p()
    for slot in (-1, 0, 1):
        assert L.ccd_enc_slot_bytes(h, slot, C.byref(out)) == ERR_ARG
        assert L.ccd_enc_slot_payload(h, slot, C.byref(dev)) == ERR_ARG
    assert L.ccd_enc_run(h, None) == 0 and L.ccd_enc_wait(h, None) == 0  # an empty handle runs nothing
    # the handle stays usable
    assert enc.add(arch, nn, lat) == 0
    assert L.ccd_enc_slot_bytes(h, 0, C.byref(out)) == ERR_ARG  # not run yet
    enc.run()
    enc.wait()
    assert enc.bytes(0) == want
    assert L.ccd_enc_slot_bytes(h, 0, None) == ERR_ARG and L.ccd_enc_slot_payload(h, 0, None) == ERR_ARG
    assert L.ccd_enc_slot_bytes(h, 1, C.byref(out)) == ERR_ARG
    enc.close()


@pytest.mark.gpu
def test_handle_semantics(gpu, oracle):
    from cool_chic_amd import writer

    arch, nn, lat, want = _rgb192(oracle)
    bs, z, _ = load_golden("hq192")
    hdr2, nn2, lat2 = _cool_chics(oracle, bs)[0]
    arch2 = writer.parse_cc_header(hdr2)
    enc = gpu(0)
    enc.add(arch, nn, lat)
    enc.run(); enc.wait()
    first = enc.bytes(0)
    enc.run(); enc.wait()
    assert enc.bytes(0) == first == want  # a second run gives the same bytes
    assert enc.add(arch2, nn2, _fixture_latents(z, arch2, 0)) == 1  # slots added after a run ...
    enc.run(); enc.wait()
    assert enc.bytes(1) == hdr2 + nn2 + lat2 and enc.bytes(0) == want  # ... are encoded by the next one
    enc.close()


@pytest.mark.gpu
def test_two_handles_from_two_threads(gpu, oracle):
    import torch

    from cool_chic_amd import writer

    arch, nn, lat, want = _rgb192(oracle)
    bs, z, _ = load_golden("kodim14")
    hdr2, nn2, lat2 = _cool_chics(oracle, bs)[0]
    arch2 = writer.parse_cc_header(hdr2)
    jobs = [[(arch, nn, lat, want)] * 3, [(arch2, nn2, _fixture_latents(z, arch2, 0), hdr2 + nn2 + lat2)] * 2]
    results = [None, None]

    def work(k):
        try:
            st = torch.cuda.Stream()
            enc = gpu(0)
            ok = True
            for _ in range(3):
                for a, n_, l_, _w in jobs[k]:
                    enc.add(a, n_, l_)
                enc.run(st.cuda_stream)
                enc.wait(st.cuda_stream)
                ok = ok and all(enc.bytes(s) == jobs[k][s % len(jobs[k])][3] for s in range(len(enc)))
            enc.close()
            results[k] = ok
        except Exception as e:  # noqa: BLE001
            results[k] = e

    ts = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert results == [True, True], results


@pytest.mark.gpu
def test_poisoned_device_latent_is_an_error_return_for_that_slot_only(gpu, oracle):
    import torch

    from cool_chic_amd import DecodeBatch
    from cool_chic_amd._lib import CcdError, lib
    from cool_chic_amd.batch import _DevArray

    names = ["rgb192", "hq192", "mop192"]
    ccs = [_cool_chics(oracle, load_golden(n)[0])[0] for n in names]
    dec = DecodeBatch(0)
    for hdr, nn, lat in ccs:
        dec.add(hdr, nn, lat, 0, 0)
    dec.run(); dec.wait()
    h1 = dec.header(1)
    ptr = lib().ccd_batch_latent(dec._h, 1, 2)
    plane = torch.as_tensor(_DevArray(ptr, (h1.grid_h[2], h1.grid_w[2]), "|i1", dec), device="cuda")
    plane.fill_(64)
    torch.cuda.synchronize()
    enc = gpu(0)
    for s in range(3):
        enc.add_from_decode(dec, s)
    enc.run()
    with pytest.raises(CcdError) as e:
        enc.wait()
    assert e.value.code == ERR_VALUE
    assert enc.slot_status(1)[0] == ERR_VALUE and enc.slot_status(0)[0] == 0 and enc.slot_status(2)[0] == 0
    with pytest.raises(CcdError):
        enc.bytes(1)
    for s in (0, 2):
        assert enc.bytes(s) == b"".join(ccs[s]), names[s]
    enc.close(); dec.close()
