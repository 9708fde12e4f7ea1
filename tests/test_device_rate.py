"""The device rate meter (ccd_enc_measure, EncodeBatch.measure / rate / rate_map) against the oracle's
intervals: a symbol whose interval has width w out of 2^24 costs 24 - log2(w) bits.

The CPU reference of a cool-chic (header, NN payload, latent payload): oracle.decode_coolchic(stop_after_entropy=True) gives
the latents and the (mu, scale) table indices in DECODE order (raster when W <= 9, else sorted by (x + 10 y, y));
oracle.laplace_bounds gives (left, right), called once per unique (mu, scale, symbol); the sums are numpy float64.

Tolerance of a sum of n terms: n * 24 * 2^-48.  Every term is at most 24; a few ulps of the device's log2 and of the
summation stay under 16 ulps of 24 (16 * 2^-52 * 24 = 24 * 2^-48) per term.  Integer sums are exact."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_golden

ERR_VALUE, ERR_ARG = -2, -7
ENTRY_POINTS = ["ccd_enc_measure", "ccd_enc_slot_rate", "ccd_enc_slot_rate_map"]
TERM_TOL = 24.0 * 2.0 ** -48


def _cool_chics(oracle, bs):
    _, frames = oracle.split_stream(bs)
    return [cc for _, ccs in frames for cc in ccs]


_REF = {}


def _reference(oracle, hdr, nn, lat):
    """{"latent": [int8 (h, w)], "width": [int64 (h, w), raster], "bits": [float64 (h, w)]}; computed once per cool-chic."""
    key = (hdr, nn, lat)
    if key in _REF:
        return _REF[key]
    r = oracle.decode_coolchic(hdr, nn, lat, stop_after_entropy=True)
    widths, planes = [], []
    for g in range(r["n_grids"]):
        h, w = r["grid_hw"][g]
        yy, xx = np.mgrid[0:h, 0:w]
        y, x = yy.ravel(), xx.ravel()
        order = np.arange(h * w) if w <= 9 else np.lexsort((y, x + 10 * y))  # raster index of the k-th decoded pixel
        ms = r["mu_scale_idx"][g].astype(np.int64)
        sym = r["latent"][g].ravel()[order].astype(np.int64)
        triple = (ms[:, 0] << 24) | (ms[:, 1] << 8) | (sym + 64)
        uniq, inv = np.unique(triple, return_inverse=True)
        wu = np.empty(len(uniq), np.int64)
        for k, t in enumerate(uniq.tolist()):
            left, right = oracle.laplace_bounds(t >> 24, (t >> 8) & 0xFFFF, (t & 0xFF) - 64)
            wu[k] = right - left
        width = np.empty(h * w, np.int64)
        width[order] = wu[inv]
        assert width.min(initial=1) >= 1 and width.max(initial=1) <= 1 << 24
        widths.append(width.reshape(h, w))
        planes.append(24.0 - np.log2(width.astype(np.float64)).reshape(h, w))
    _REF[key] = {"latent": [np.ascontiguousarray(a) for a in r["latent"]], "width": widths, "bits": planes}
    return _REF[key]


def _check_rate(rate, ref, what):
    """Test 1's rules: symbol counts and width sums exact, bits within n * 24 * 2^-48 of the float64 reference."""
    assert rate.status == 0, what
    n_grids = len(ref["width"])
    assert len(rate.bits) == len(rate.sum_width) == len(rate.n_symbols) == n_grids, what
    worst = 0.0
    for g in range(n_grids):
        n = ref["width"][g].size
        assert int(rate.n_symbols[g]) == n, (what, g)
        assert int(rate.sum_width[g]) == int(ref["width"][g].sum()), (what, g)
        want = float(ref["bits"][g].sum())
        dev = abs(float(rate.bits[g]) - want)
        worst = max(worst, dev / (n * TERM_TOL))
        assert dev <= n * TERM_TOL, (what, g, float(rate.bits[g]), want)
    n_all = sum(a.size for a in ref["width"])
    want = math.fsum(float(p.sum()) for p in ref["bits"])
    dev = abs(rate.total_bits - want)
    assert dev <= n_all * TERM_TOL, (what, rate.total_bits, want)
    return max(worst, dev / (n_all * TERM_TOL)), n_all, want


def _bits64(rate):
    return np.concatenate([rate.bits, [rate.total_bits]]).astype(np.float64).view(np.uint64).tolist()


# ---- CPU -------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_exported():
    from cool_chic_amd import _lib

    with open(os.path.join(ROOT, "include", "ccd.h")) as f:
        header = f.read()
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert name + "(" in header, name
        assert name in _lib.SIGNATURES, name
        assert getattr(L, name) is not None
    assert "ccd_enc_rate;" in header
    from cool_chic_amd.encoder import EncodeBatch

    assert all(hasattr(EncodeBatch, m) for m in ("measure", "rate", "rate_map"))


def test_null_arguments_are_argument_errors_without_a_device():
    from cool_chic_amd._lib import EncRate, lib

    L = lib()
    out = EncRate()
    dev = C.c_void_p()
    assert L.ccd_enc_measure(None, None, 0) == ERR_ARG
    assert L.ccd_enc_measure(None, None, 1) == ERR_ARG
    assert L.ccd_enc_slot_rate(None, 0, C.byref(out)) == ERR_ARG
    assert L.ccd_enc_slot_rate(None, 0, None) == ERR_ARG
    assert L.ccd_enc_slot_rate_map(None, 0, 0, C.byref(dev)) == ERR_ARG and not dev.value
    assert L.ccd_enc_slot_rate_map(None, 0, 0, None) == ERR_ARG


def test_result_struct_matches_the_header():
    """The ctypes mirror of ccd_enc_rate has the layout the header declares (CCD_MAX_GRIDS entries per array)."""
    from cool_chic_amd._lib import MAX_GRIDS, EncRate

    assert C.sizeof(EncRate) == 8 + 3 * 8 * MAX_GRIDS + 8 + 16
    assert EncRate.total_bits.offset == 8 + 3 * 8 * MAX_GRIDS


def test_cli_lists_the_rate_breakdown():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "cc_decode.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "--rate-breakdown" in r.stdout


# ---- GPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cool_chic_amd import EncodeBatch, _lib

    _lib.lib()
    return EncodeBatch


def _fixture_jobs(oracle):
    """[(name, arch, nn, reference)]: rgb192 is slot 3; 10- and 5-grid slots, the W <= 9 branch, one-block grids, tail lanes."""
    from cool_chic_amd import writer

    jobs = []
    for name in ["odd18x65", "odd100x37", "kodim14", "rgb192", "vid3_ldp"]:
        for i, (hdr, nn, lat) in enumerate(_cool_chics(oracle, load_golden(name)[0])):
            jobs.append((f"{name}/{i}", writer.parse_cc_header(hdr), nn, _reference(oracle, hdr, nn, lat)))
    assert len(jobs) == 9 and jobs[3][0] == "rgb192/0"
    assert {j[1].n_grids for j in jobs} == {10, 5}
    return jobs


@pytest.fixture(scope="module")
def measured(gpu, oracle):
    """The nine reference-encoded cool-chics in ONE handle, measured once: (handle, jobs, rates)."""
    jobs = _fixture_jobs(oracle)
    enc = gpu(0)
    for _, arch, nn, ref in jobs:
        enc.add(arch, nn, ref["latent"])
    enc.measure()
    enc.wait()
    rates = [enc.rate(s) for s in range(len(jobs))]
    yield enc, jobs, rates
    enc.close()


@pytest.mark.gpu
def test_parity_on_the_reference_encoded_fixtures(measured):
    _, jobs, rates = measured
    min_width = 1 << 24
    for (name, arch, nn, ref), rate in zip(jobs, rates):
        worst, n, want = _check_rate(rate, ref, name)
        assert rate.n_bytes_nn == len(nn) and rate.n_bytes_header == arch.n_bytes_header
        min_width = min(min_width, min(int(w.min()) for w in ref["width"]))
        print(f"{name}: {n} symbols, model bits {rate.total_bits:.3f} (reference {want:.3f}), worst deviation {worst:.3g} of the bound")
    assert min_width == 1  # the 24-bit symbol is among the cases


@pytest.mark.gpu
def test_rate_map(gpu, oracle):
    import torch

    from cool_chic_amd import writer

    enc = gpu(0)
    refs = []
    for name in ("rgb192", "odd18x65"):
        hdr, nn, lat = _cool_chics(oracle, load_golden(name)[0])[0]
        refs.append(_reference(oracle, hdr, nn, lat))
        enc.add(writer.parse_cc_header(hdr), nn, refs[-1]["latent"])
    enc.measure(rate_map=True)
    enc.wait()
    n_24 = 0
    for s, ref in enumerate(refs):
        rate = enc.rate(s)
        _check_rate(rate, ref, s)
        for g, want in enumerate(ref["bits"]):
            dev = enc.rate_map(s, g)
            assert dev.__cuda_array_interface__["shape"] == want.shape and dev.__cuda_array_interface__["typestr"] == "<f4"
            got = torch.as_tensor(dev, device="cuda").cpu().numpy()
            assert got.dtype == np.float32 and got.shape == want.shape
            assert np.abs(got.astype(np.float64) - want.astype(np.float32).astype(np.float64)).max() <= 2e-6, (s, g)
            assert abs(float(got.astype(np.float64).sum()) - float(rate.bits[g])) <= want.size * 2e-6, (s, g)
            one = ref["width"][g] == 1
            assert (got[one] == np.float32(24.0)).all(), (s, g)
            n_24 += int(one.sum())
    assert n_24 > 0
    enc.close()


@pytest.mark.gpu
def test_a_slot_gives_the_same_bits_alone_and_in_a_batch(gpu, measured):
    _, jobs, rates = measured
    name, arch, nn, ref = jobs[3]
    alone = []
    for _ in range(2):
        enc = gpu(0)
        enc.add(arch, nn, ref["latent"])
        enc.measure()
        enc.wait()
        alone.append(_bits64(enc.rate(0)))
        enc.close()
    assert alone[0] == alone[1] == _bits64(rates[3])


def _perturbed_networks(arch, nn_ints, want=3, seed=0):
    """`want` networks whose ARM weights differ from nn_ints by +-1 in six places and that writer.encode_network accepts:
    [(arch with its own nn_n_bytes, payload, integers)].  The caller keeps those the oracle reads back unchanged; seed 0
    yields three such on the CPU."""
    from cool_chic_amd import writer
    from cool_chic_amd._lib import CCHeader

    rng = np.random.default_rng(seed)
    n_arm_w = writer.network_layout(arch)[0]
    out = []
    for _ in range(4 * want):
        values = np.array(nn_ints, np.int64)
        where = rng.choice(n_arm_w, size=6, replace=False)
        values[where] += rng.choice([-1, 1], size=6)
        a = CCHeader.from_buffer_copy(bytes(arch))
        try:
            nn = writer.encode_network(a, values)
        except Exception:  # noqa: BLE001  (a value the Exp-Golomb orders of the header cannot carry)
            continue
        out.append((a, nn, values))
        if len(out) == want:
            break
    return out


@pytest.mark.gpu
def test_candidates_that_share_latents(gpu, oracle):
    from cool_chic_amd import DecodeBatch, writer
    from cool_chic_amd._lib import lib

    bs, z, _ = load_golden("rgb192")
    hdr, nn, lat = _cool_chics(oracle, bs)[0]
    arch = writer.parse_cc_header(hdr)
    ref0 = _reference(oracle, hdr, nn, lat)
    nn_ints = oracle.decode_coolchic(hdr, nn, lat, stop_after_entropy=True)["nn_ints"]
    candidates = [(arch, nn, ref0)]
    for a, nn_k, values in _perturbed_networks(arch, nn_ints):
        # the host writer's cool-chic for this network and the SAME latents, then the reference from its own bytes
        cc = writer.encode_coolchic(a, nn_k, ref0["latent"])
        h2 = writer.parse_cc_header(cc)
        p, q = h2.n_bytes_header, h2.n_bytes_header + h2.nn_n_bytes
        back = oracle.decode_coolchic(cc[:p], cc[p:q], cc[q:], stop_after_entropy=True)
        if not np.array_equal(back["nn_ints"], values):
            continue  # encode_network did not round-trip this one
        assert all(np.array_equal(x, y) for x, y in zip(back["latent"], ref0["latent"]))
        candidates.append((h2, cc[p:q], _reference(oracle, cc[:p], cc[p:q], cc[q:])))
    assert len(candidates) == 4
    dec = DecodeBatch(0)
    dec.add(hdr, nn, lat, 0, 0)
    dec.run(); dec.wait()
    ptrs = [lib().ccd_batch_latent(dec._h, 0, g) for g in range(arch.n_grids)]
    enc = gpu(0)
    for a, nn_k, _ in candidates:
        enc.add_device(a, nn_k, ptrs, owner=dec)
    enc.measure()
    enc.wait()
    totals = []
    for s, (_, _, ref) in enumerate(candidates):
        rate = enc.rate(s)
        _check_rate(rate, ref, s)
        totals.append(rate.total_bits)
    print("candidate totals:", totals)
    assert len(set(totals)) > 1
    enc.close(); dec.close()


def _coder_condition(enc, slot, total_bits):
    status, counters = enc.slot_status(slot)
    assert status == 0
    extra = int(counters[1]) - math.ceil(total_bits / 32)
    assert 0 <= extra <= 3, (slot, int(counters[1]), total_bits)
    return extra


@pytest.mark.gpu
def test_agreement_with_the_coder(gpu, measured):
    enc, jobs, rates = measured
    enc.run()
    enc.wait()
    extras = [_coder_condition(enc, s, rates[s].total_bits) for s in range(len(jobs))]
    print("payload words - ceil(model bits / 32):", extras)
    for s in range(len(jobs)):  # still readable, and unchanged by the run
        assert _bits64(enc.rate(s)) == _bits64(rates[s]) and enc.rate(s).sum_width.tolist() == rates[s].sum_width.tolist()
    # the other order on a fresh handle
    other = gpu(0)
    for _, arch, nn, ref in jobs:
        other.add(arch, nn, ref["latent"])
    other.run()
    other.wait()
    words = [int(other.slot_status(s)[1][1]) for s in range(len(jobs))]
    other.measure()
    other.wait()
    for s in range(len(jobs)):
        assert _bits64(other.rate(s)) == _bits64(rates[s]), s
        assert int(other.slot_status(s)[1][1]) == words[s] == int(enc.slot_status(s)[1][1])  # and the run's results stay
    other.close()


@pytest.mark.gpu
def test_poisoned_device_latent_is_that_slots_error_only(gpu, oracle):
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
    enc.measure(rate_map=True)
    with pytest.raises(CcdError) as e:
        enc.wait()
    assert e.value.code == ERR_VALUE
    bad = enc.rate(1)
    assert bad.status == ERR_VALUE and bad.total_bits == 0.0 and not bad.bits.any() and not bad.sum_width.any()
    with pytest.raises(CcdError):
        enc.rate_map(1, 0)
    for s in (0, 2):
        _check_rate(enc.rate(s), _reference(oracle, *ccs[s]), names[s])
    enc.close(); dec.close()


@pytest.mark.gpu
def test_argument_checks_on_a_live_handle(gpu, oracle):
    from cool_chic_amd import writer
    from cool_chic_amd._lib import EncRate, lib

    L = lib()
    hdr, nn, lat = _cool_chics(oracle, load_golden("odd18x65")[0])[0]
    arch, ref = writer.parse_cc_header(hdr), _reference(oracle, hdr, nn, lat)
    enc = gpu(0)
    h = enc._h
    out, dev = EncRate(), C.c_void_p()
    assert L.ccd_enc_measure(h, None, 0) == 0 and L.ccd_enc_wait(h, None) == 0  # an empty handle measures nothing
    assert L.ccd_enc_slot_rate(h, 0, C.byref(out)) == ERR_ARG
    enc.add(arch, nn, ref["latent"])
    assert L.ccd_enc_slot_rate(h, 0, C.byref(out)) == ERR_ARG  # before any measure
    assert L.ccd_enc_slot_rate_map(h, 0, 0, C.byref(dev)) == ERR_ARG
    enc.run(); enc.wait()
    assert L.ccd_enc_slot_rate(h, 0, C.byref(out)) == ERR_ARG  # a run is not a measure
    enc.measure(); enc.wait()
    assert L.ccd_enc_slot_rate(h, 0, C.byref(out)) == 0 and out.n_grids == arch.n_grids
    assert L.ccd_enc_slot_rate(h, 0, None) == ERR_ARG
    for slot in (-1, 1):
        assert L.ccd_enc_slot_rate(h, slot, C.byref(out)) == ERR_ARG
    assert L.ccd_enc_slot_rate_map(h, 0, 0, C.byref(dev)) == ERR_ARG and not dev.value  # measured without a map
    enc.measure(rate_map=True); enc.wait()
    assert L.ccd_enc_slot_rate_map(h, 0, 0, C.byref(dev)) == arch.grid_h[0] * arch.grid_w[0] and dev.value
    for grid in (-1, arch.n_grids):
        assert L.ccd_enc_slot_rate_map(h, 0, grid, C.byref(dev)) == ERR_ARG
    assert L.ccd_enc_slot_rate_map(h, 1, 0, C.byref(dev)) == ERR_ARG
    assert L.ccd_enc_slot_rate_map(h, 0, 0, None) == ERR_ARG
    enc.add(arch, nn, ref["latent"])  # a slot no measure covered yet
    assert L.ccd_enc_slot_rate(h, 1, C.byref(out)) == ERR_ARG
    enc.measure(); enc.wait()
    assert L.ccd_enc_slot_rate_map(h, 0, 0, C.byref(dev)) == ERR_ARG  # the last measure had no map
    _check_rate(enc.rate(1), ref, "added after a measure")
    enc.close()


@pytest.mark.gpu
def test_rate_breakdown_of_a_video(gpu, oracle, tmp_path):
    from cool_chic_amd import writer
    from cool_chic_amd.bitstream.decode import decode_video
    from cool_chic_amd.bitstream.header import VideoHeader

    path = os.path.join(GOLDEN, "vid3_ldp.cool")
    table = tmp_path / "rate.tsv"
    before = set(os.listdir(tmp_path))
    frames = decode_video(path, device=0)
    assert set(os.listdir(tmp_path)) == before  # without the path no file is written
    frames2 = decode_video(path, device=0, rate_breakdown_path=str(table))
    assert set(frames2) == set(frames) and table.exists()
    lines = table.read_text().splitlines()
    cols = lines[0].split("\t")
    assert cols == ["display", "cool_chic", "grid", "h", "w", "symbols", "model_bits", "bytes_header", "bytes_nn", "bytes_latent"]
    rows = [dict(zip(cols, ln.split("\t"))) for ln in lines[1:]]
    # the same cool-chics through EncodeBatch
    bs = open(path, "rb").read()
    vh = VideoHeader()
    vh.read_header(bs)
    structure = vh.get_coding_structure()
    _, parsed = oracle.split_stream(bs)
    enc = gpu(0)
    keys = []
    for k, (_fh, ccs) in enumerate(parsed):
        for i, (hdr, nn, lat) in enumerate(ccs):
            enc.add(writer.parse_cc_header(hdr), nn, _reference(oracle, hdr, nn, lat)["latent"])
            keys.append((structure[k]["display_order"], i, writer.parse_cc_header(hdr)))
    enc.measure(); enc.wait()
    n_rows = 0
    for s, (d, i, arch) in enumerate(keys):
        rate = enc.rate(s)
        mine = [r for r in rows if (int(r["display"]), int(r["cool_chic"])) == (d, i)]
        assert len(mine) == arch.n_grids + 1
        n_rows += len(mine)
        for g in range(arch.n_grids):
            r = mine[g]
            assert (int(r["grid"]), int(r["h"]), int(r["w"]), int(r["symbols"])) == (g, arch.grid_h[g], arch.grid_w[g], int(rate.n_symbols[g]))
            assert float(r["model_bits"]) == float(rate.bits[g])
        r = mine[-1]
        assert r["grid"] == "all" and float(r["model_bits"]) == rate.total_bits and int(r["symbols"]) == int(rate.n_symbols.sum())
        assert (int(r["bytes_header"]), int(r["bytes_nn"]), int(r["bytes_latent"])) == (arch.n_bytes_header, arch.nn_n_bytes, arch.n_bytes_latent)
        assert 0 <= arch.n_bytes_latent // 4 - math.ceil(rate.total_bits / 32) <= 3 and arch.n_bytes_latent % 4 == 0
    assert n_rows == len(rows) and len(keys) == 5
    enc.close()
