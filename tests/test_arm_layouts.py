"""ARM and IFCE layouts no preset has, through the device writer, the rate meter, the rate deltas and the decoder (DESIGN.md
section 4.10 "What pins encode_pixel_model"; the cases: tests/arm_layouts.py).

CPU half: the case list holds every class it is there for (inventory), every case decodes in the oracle to the latents it was
written from, one changed parameter at the END of every weight array changes the host writer's bytes (so a kernel that dropped
the last row, column, channel or grid would fail the byte comparison), and the range coder restated with counters reproduces
the host writer's payloads and finds both seal forms and both resolutions of an inverted run among the tiny cases.
GPU half: the 91 shapes of tests/golden/arm_sweep.npz and the crafted cases through EncodeBatch.run / measure / measure_deltas
and DecodeBatch, against the fixture's bytes, the host writer's bytes and the oracle's intervals.  IFCE beyond
ifce_resolution (0, 2) is pinned oracle <-> host writer <-> device only: no reference-decoded fixture has it."""
import hashlib

import numpy as np
import pytest

import arm_layouts as al
from conftest import load_arm_sweep

ERR_UNSUPPORTED = -4
SPECS = al.specs()
NAMES = [s[0] for s in SPECS]
LAYOUT_NAMES = [s[0] for s in SPECS if s[1] != "tiny"]
PLACEMENT_NAMES = [s[0] for s in SPECS if s[1] == "placement"]
TINY_NAMES = [s[0] for s in SPECS if s[1] == "tiny"]
WIDE_NAMES = [s[0] for s in SPECS if s[2][0] + s[2][1] > 64]  # more than 64 KB of LDS in the encoder kernels
# what every placement must give at both sizes (rgb192's ten grids; 5, 7 and 9 are the hyperlatent ones)
PLACEMENT_FEATURES = {(0, 15): [9, 8, 7, 6, 5, 4, 3, 2, 1, 1], (3, 15): [0, 0, 0, 6, 5, 4, 3, 2, 1, 1], (1, 1): [0, 8, 0, 0, 0, 0, 0, 0, 0, 0],
                      (4, 4): [0, 0, 0, 0, 5, 4, 0, 0, 0, 0]}


def _fin(arch):
    return [int(arch.input_features_ifce[g]) for g in range(arch.n_grids)]


# ---- CPU -------------------------------------------------------------------------------------------------------------
def test_the_drawing_rule_still_writes_the_committed_sweep():
    """arm_layouts.build_stream is the rule tests/golden/gen/make_arm_sweep.py wrote arm_sweep.npz with: its 91 streams, byte for
    byte (the reference-decoded hashes of the fixture stay the expected outputs of these bytes)."""
    d_hdr, d_ints, d_lat = al.donor()
    sweep = load_arm_sweep()
    configs = [(dim, nh, n_ifce) for dim in [3, 4, 8, 12, 14, 16, 20, 24, 26, 28, 32] for nh in range(4) for n_ifce in (0, 2) if dim - n_ifce >= 1]
    configs += [(29, 7, 0), (32, 7, 2), (31, 6, 2)]
    assert len(configs) == len(sweep) == 91
    for i, (dim, nh, n_ifce) in enumerate(configs):
        stream, _, _ = al.build_stream(d_hdr, d_ints, d_lat, dim, nh, n_ifce, seed=4000 + i)
        assert stream == sweep[f"d{dim}_h{nh}_i{n_ifce}"][0], (dim, nh, n_ifce)


def test_inventory():
    cases = al.cases()
    assert 40 <= len(cases) <= 55 and len({c.name for c in cases}) == len(cases)
    arch = [c.arch for c in cases]
    dims = {a.total_context_arm for a in arch}
    assert any(d % 2 for d in dims - {1}) and any(d % 2 == 0 for d in dims)
    assert 1 in dims and 64 in dims and max(dims) == 71 and {65, 70} <= dims
    assert {a.n_hidden_layers_arm for a in arch} == set(range(8))
    with_ifce = [a for a in arch if any(_fin(a))]
    assert any(a.output_feature_ifce % 2 for a in with_ifce) and any(a.output_feature_ifce == 7 for a in with_ifce)
    assert any(a.output_feature_ifce == 0 and not any(_fin(a)) for a in arch)
    assert any(_fin(a)[-1] > 0 for a in arch), "IFCE on the last grid"
    assert any(a.is_hyperlatent[g] and al.has_sources(a, g) for a in arch for g in range(a.n_grids)), "IFCE on a hyperlatent grid"
    assert any(al.has_sources(a, g) and a.grid_w[g] <= 9 and a.grid_h[g] * a.grid_w[g] > 1 for a in arch for g in range(a.n_grids)), "IFCE on a raster grid"
    assert any(al.has_sources(a, g) and a.grid_w[g] > 9 for a in arch for g in range(1, a.n_grids)), "IFCE on a coarse wavefront grid"
    assert any(_fin(a)[g] > 0 and _fin(a)[g - 1] == 0 for a in arch for g in range(1, a.n_grids)), "IFCE below a grid without"
    # a grid whose neighbour has the same size (latent grid and hyperlatent grid of one level), both with features
    assert any(al.has_sources(a, g) and al.has_sources(a, g + 1) and (a.grid_h[g], a.grid_w[g]) == (a.grid_h[g + 1], a.grid_w[g + 1])
               and a.grid_h[g] * a.grid_w[g] > 1 for a in arch for g in range(a.n_grids - 1))
    n_sym = [int(a.n_symbols) for a in arch]
    assert any(n < 64 for n in n_sym) and 64 in n_sym and 10 in n_sym
    assert {0, 1, 63} <= {n % 64 for n in n_sym}
    assert {63, 64, 65, 127, 128, 255, 256} <= set(n_sym)
    for c in cases:
        assert c.arch.n_grids == 10 and int(c.arch.n_symbols) == sum(a.size for a in c.latents), c.name
        if c.kind == "placement":
            assert _fin(c.arch) == PLACEMENT_FEATURES[c.placement], c.name
        if c.kind == "tiny":
            assert all(f > 0 for f in _fin(c.arch)) if c.placement else not any(_fin(c.arch)), c.name
    # -64 next to 63 in a few of them, the widest ARM and a tiny one among them
    extreme = [c for c in cases if any((a[:, :-1].astype(int) - a[:, 1:] == -127).any() for a in c.latents if a.shape[1] > 1)]
    assert len(extreme) >= 4 and any(c.arch.total_context_arm == 71 for c in extreme) and any(c.kind == "placement" for c in extreme)
    # the decoder takes all of them but the two whose ARM does not fit the generic kernel's LDS; two of more than 64 inputs stay
    assert sorted(c.arch.total_context_arm for c in cases if not al.device_decodable(c.arch)) == [64, 71]
    assert sorted(c.arch.total_context_arm for c in cases if al.device_decodable(c.arch) and c.arch.total_context_arm >= 64) == [65, 70]
    # every placement has a case with an odd dim and one with 7 features, at both sizes
    for res in PLACEMENT_FEATURES:
        mine = [c for c in cases if c.kind == "placement" and c.placement == res]
        assert {c.img_size for c in mine} == {(18, 65), (37, 100)}, res
        for size in ((18, 65), (37, 100)):
            assert any(c.arch.total_context_arm % 2 for c in mine if c.img_size == size)
            assert any(c.arch.output_feature_ifce == 7 for c in mine if c.img_size == size)


def test_kernel_classes():
    """ccd_network_kernel_class: the pipelined entropy kernel for every case below 64 ARM inputs, the generic one from 64 on."""
    from cool_chic_amd._lib import lib

    for c in al.cases():
        cls = lib().ccd_network_kernel_class(c.hdr, len(c.hdr), c.nn, len(c.nn))
        assert cls >= 0 and bool(cls & 1) == (c.arch.total_context_arm < 64), (c.name, cls)


@pytest.mark.parametrize("name", NAMES)
def test_round_trip_in_the_oracle(oracle, name):
    c = al.case(name)
    r = al.entropy(oracle, c)
    assert r["n_symbols"] == c.arch.n_symbols and r["input_features_ifce"] == _fin(c.arch)
    for g, (got, want) in enumerate(zip(r["latent"], c.latents)):
        assert np.array_equal(got, want), (name, g)


def _sensitive_parameters(arch):
    """[(what, index into the transmitted integers)]: the LAST entry of every weight array encode_pixel_model indexes.  Stream
    order (ccd_format.cpp::decode_network): arm.w = hidden layers [out][in], output layer [2][in], stabiliser [2][in]; arm.b;
    ifce.w = per grid with features [out][in]; ifce.b = per grid with features [out]."""
    from cool_chic_amd import writer

    n = writer.network_layout(arch)
    dim, nh, n_if = arch.total_context_arm, arch.n_hidden_layers_arm, arch.output_feature_ifce
    out = [("layer %d: last input -> last hidden unit" % l, (l + 1) * dim * dim - 1) for l in range(nh)]
    out.append(("output layer: last hidden unit -> log-scale", nh * dim * dim + 2 * dim - 1))
    assert arch.linear_stabiliser_arm
    out.append(("stabiliser: last input -> log-scale", nh * dim * dim + 4 * dim - 1))
    assert n[0] == nh * dim * dim + 4 * dim
    fin = _fin(arch)
    if any(fin):
        src = max(g for g in range(arch.n_grids) if al.has_sources(arch, g))
        at = n[0] + n[1] + sum(n_if * fin[g] for g in range(src)) + n_if * fin[src] - 1
        out.append(("IFCE of grid %d: last source channel -> last feature" % src, at))
        last = max(g for g in range(arch.n_grids) if fin[g] > 0)
        assert n[2] == sum(n_if * f for f in fin) and n[3] == n_if * sum(f > 0 for f in fin)
        out.append(("IFCE of grid %d: bias of the last feature" % last, n[0] + n[1] + n[2] + n[3] - 1))
    return out


@pytest.mark.parametrize("name", LAYOUT_NAMES)
def test_last_parameters_are_visible_in_the_bytes(oracle, name):
    """One parameter moved by 64 quantisation steps, everything else and the latents as they are: another latent payload."""
    from cool_chic_amd import writer
    from cool_chic_amd._lib import CCHeader

    c = al.case(name)
    ints = al.entropy(oracle, c)["nn_ints"]
    assert len(ints) == sum(writer.network_layout(c.arch))
    for what, at in _sensitive_parameters(c.arch):
        moved = np.array(ints, np.int64)
        moved[at] += 64
        a = CCHeader.from_buffer_copy(bytes(c.arch))
        cc = writer.encode_coolchic(a, writer.encode_network(a, moved), c.latents)
        h2 = writer.parse_cc_header(cc)
        payload = cc[h2.n_bytes_header + h2.nn_n_bytes:]
        assert payload != c.payload, (name, what)
        back = oracle.decode_coolchic(cc[:h2.n_bytes_header], cc[h2.n_bytes_header:h2.n_bytes_header + h2.nn_n_bytes], payload, stop_after_entropy=True)
        assert np.array_equal(back["nn_ints"], moved), (name, what)  # the payload carried the moved value
        assert all(np.array_equal(x, y) for x, y in zip(back["latent"], c.latents)), (name, what)


def test_chain_inventory(oracle):
    """The range coder restated with counters (arm_layouts.chain_count) writes the host writer's payload of every case; among the
    tiny cases it seals with one word and with two, resolves inverted runs with a carry and without, and holds a run of two
    words.  The longest run in any case is 2 words; a run longer than 65 words - the second round of the
    lane-strided fill of flush_inverted - needs ~65 consecutive renormalisations that leave the interval straddling a 2^32
    boundary and is not reachable by seeded inputs."""
    cases = al.cases()
    for c in cases:
        ch = al.chain(oracle, c)
        assert ch.payload == c.payload and ch.words * 4 == len(c.payload), c.name
        assert ch.runs == ch.carry + ch.plain
    tiny = [al.chain(oracle, c) for c in cases if c.kind == "tiny"]
    assert len(tiny) == len(TINY_NAMES) == 20
    assert {ch.seal_words for ch in tiny} == {1, 2}
    assert any(ch.carry for ch in tiny) and any(ch.plain for ch in tiny)
    assert max(ch.longest for ch in tiny) >= 2
    # the two-word seal right at the edges of the device coder's 64-symbol chunks
    two = {int(c.arch.n_symbols) for c in cases if al.chain(oracle, c).seal_words == 2}
    assert {63, 64, 65} <= two, two
    print("longest inverted run:", max(al.chain(oracle, c).longest for c in cases), "words")


# ---- GPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cool_chic_amd import EncodeBatch, _lib

    _lib.lib()
    return EncodeBatch


def _narrow():
    """The crafted cases whose encoder kernels stay inside the default 64 KB of LDS (dim <= 64); the wider ones have tests of
    their own."""
    return [c for c in al.cases() if c.name not in WIDE_NAMES]


def _rate_reference(oracle, c):
    from test_device_rate import _reference

    return _reference(oracle, c.hdr, c.nn, c.payload)


def _check_written(enc, slot, c, oracle):
    """Bytes = the host writer's, inside the payload bound, counters = the Python restatement's."""
    from test_device_encoder import _check_bound, _device_bytes

    got = enc.bytes(slot)
    assert got == c.cc, c.name
    n = _check_bound(enc, slot, c.arch)
    assert n == len(c.payload) and bytes(_device_bytes(enc.payload(slot))) == c.payload, c.name
    status, counters = enc.slot_status(slot)
    ch = al.chain(oracle, c)
    assert status == 0 and tuple(int(v) for v in counters[1:5]) == (ch.words, ch.runs, ch.carry, ch.plain), (c.name, counters[:5], ch[1:])


@pytest.mark.gpu
def test_sweep_through_the_writer_and_the_meter(gpu, oracle):
    """The 91 ARM shapes of arm_sweep.npz in ONE EncodeBatch: from the oracle-decoded latents (= what the REFERENCE decoder
    decoded: sha256 per grid in the fixture) run() writes the fixture's cool-chic bytes, and measure() in the same handle gives
    the oracle's widths exactly and its bits within test_device_rate's bound."""
    from cool_chic_amd import writer
    from test_device_encoder import _check_bound
    from test_device_rate import _check_rate, _reference

    sweep = load_arm_sweep()
    enc = gpu(0)
    try:
        jobs = []
        for name, (stream, hashes) in sweep.items():
            hdr, nn, lat = oracle.split_stream(stream)[1][0][1][0]
            ref = _reference(oracle, hdr, nn, lat)
            assert [hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() for a in ref["latent"]] == hashes, name
            arch = writer.parse_cc_header(hdr)
            assert enc.add(arch, nn, ref["latent"]) == len(jobs)
            jobs.append((name, arch, hdr + nn + lat, ref))
        assert len(jobs) == 91
        enc.run()
        enc.wait()
        for s, (name, arch, want, _) in enumerate(jobs):
            assert enc.bytes(s) == want, name
            _check_bound(enc, s, arch)
        enc.measure()
        enc.wait()
        worst = max(_check_rate(enc.rate(s), ref, name)[0] for s, (name, _, _, ref) in enumerate(jobs))
        print(f"sweep: 91 slots, worst deviation {worst:.3g} of the bound")
        for s, (name, _, want, _) in enumerate(jobs):  # the measure left the run's results alone
            assert enc.bytes(s) == want, name
    finally:
        enc.close()


@pytest.mark.gpu
def test_crafted_layouts_through_the_writer(gpu, oracle):
    cases = _narrow()
    assert any(c.arch.total_context_arm == 64 for c in cases)  # exactly 64 KB: the largest launch without the opt-in
    enc = gpu(0)
    try:
        for c in cases:
            enc.add(c.arch, c.nn, c.latents)
        enc.run()
        enc.wait()
        for s, c in enumerate(cases):
            _check_written(enc, s, c, oracle)
    finally:
        enc.close()


@pytest.mark.gpu
def test_crafted_layouts_round_trip_without_the_host(gpu, oracle):
    """DecodeBatch -> add_from_decode -> the bytes that were decoded, for every crafted case that fits the default LDS of the
    encoder kernels and that the decoder takes."""
    from cool_chic_amd import DecodeBatch

    cases = [c for c in _narrow() if al.device_decodable(c.arch)]
    dec = DecodeBatch(0)
    enc = gpu(0)
    try:
        for c in cases:
            dec.add(c.hdr, c.nn, c.payload, 0, 0)
        dec.run()
        dec.wait()
        for s in range(len(cases)):
            assert enc.add_from_decode(dec, s) == s
        enc.run()
        enc.wait()
        for s, c in enumerate(cases):
            _check_written(enc, s, c, oracle)
    finally:
        enc.close()
        dec.close()


def _check_maps(enc, slot, c, ref):
    """test_device_rate.py::test_rate_map's rules; returns the number of width-1 symbols (24.0 bits exactly)."""
    import torch

    rate, n_24 = enc.rate(slot), 0
    for g, want in enumerate(ref["bits"]):
        dev = enc.rate_map(slot, g)
        assert dev.__cuda_array_interface__["shape"] == want.shape and dev.__cuda_array_interface__["typestr"] == "<f4"
        got = torch.as_tensor(dev, device="cuda").cpu().numpy()
        assert np.abs(got.astype(np.float64) - want.astype(np.float32).astype(np.float64)).max() <= 2e-6, (c.name, g)
        assert abs(float(got.astype(np.float64).sum()) - float(rate.bits[g])) <= want.size * 2e-6, (c.name, g)
        one = ref["width"][g] == 1
        assert (got[one] == np.float32(24.0)).all(), (c.name, g)
        n_24 += int(one.sum())
    return n_24


@pytest.mark.gpu
def test_crafted_layouts_through_the_meter(gpu, oracle):
    from test_device_rate import _check_rate

    cases = _narrow()
    enc = gpu(0)
    try:
        for c in cases:
            enc.add(c.arch, c.nn, c.latents)
        enc.measure(rate_map=True)
        enc.wait()
        worst, n_24 = 0.0, 0
        for s, c in enumerate(cases):
            ref = _rate_reference(oracle, c)
            worst = max(worst, _check_rate(enc.rate(s), ref, c.name)[0])
            assert enc.rate(s).n_bytes_nn == len(c.nn) and enc.rate(s).n_bytes_header == c.arch.n_bytes_header
            if c.kind == "placement":
                n_24 += _check_maps(enc, s, c, ref)
        assert n_24 > 0
        print(f"crafted layouts: {len(cases)} slots, worst deviation {worst:.3g} of the bound, {n_24} width-1 symbols in the maps")
    finally:
        enc.close()


@pytest.mark.gpu
def test_more_than_64_arm_inputs_through_the_writer_and_the_meter(gpu, oracle):
    """dim 65, 70 and 71: encode_contexts_lds_bytes is above 64 KB, so launch_encode and launch_encode_rate take their
    hipFuncSetAttribute branch; a 5-input slot in the same handle runs under the LDS size of the largest slot."""
    from test_device_rate import _check_rate

    cases = [al.case(n) for n in WIDE_NAMES] + [al.case("arm_s3_i2_h4")]
    assert sorted(c.arch.total_context_arm for c in cases) == [5, 65, 70, 71]
    enc = gpu(0)
    try:
        for c in cases:
            enc.add(c.arch, c.nn, c.latents)
        enc.run()
        enc.wait()
        for s, c in enumerate(cases):
            _check_written(enc, s, c, oracle)
        enc.measure(rate_map=True)
        enc.wait()
        for s, c in enumerate(cases):
            ref = _rate_reference(oracle, c)
            _check_rate(enc.rate(s), ref, c.name)
            _check_maps(enc, s, c, ref)
    finally:
        enc.close()


# ---- rate deltas: the rules of tests/test_rate_deltas.py on the crafted layouts -----------------------------------------
# odd dim / 0 hidden layers and one input / the four placements / two tiny ones; dim 71 (the opt-in of launch_encode_deltas)
# is a test of its own.  Oracle decodes per case: about 300 at 18 x 65 (the cap of 500 is asserted).
DELTA_NAMES = ["arm_s3_i2_h4", "arm_s1_i0_h0", "ifce0_15_18x65_s6_i3_h3", "ifce3_15_18x65_s9_i7_h6", "ifce1_1_18x65_s6_i3_h3",
               "ifce4_4_18x65_s9_i7_h6", "tiny3x13_s5_i2_h1", "tiny5x8_s6_i0_h2"]
_DELTA = {}


def _delta_case(oracle, name):
    """(test_rate_deltas._Case, [(grid, y, x, sign, reference)]) of a crafted case, once."""
    from test_rate_deltas import _Case, _positions

    if name not in _DELTA:
        c = al.case(name)
        case = _Case(oracle, name, c.hdr, c.nn, c.payload)
        assert all(np.array_equal(a, b) for a, b in zip(case.latents, c.latents))
        rng = np.random.default_rng(1234)
        checks = []
        for m in range(case.n):
            for y, x, signs in _positions(case, m, rng):
                checks += [(m, y, x, s, case.reference(m, y, x, s)) for s in signs]
        assert case.n_decodes <= 500, (name, case.n_decodes)
        _DELTA[name] = (case, checks)
    return _DELTA[name]


def _check_deltas(gpu, oracle, names):
    from test_rate_deltas import _check, _maps

    enc = gpu(0)
    try:
        for name in names:
            c = al.case(name)
            enc.add(c.arch, c.nn, c.latents)
        enc.measure_deltas()
        enc.wait()
        for s, name in enumerate(names):
            case, checks = _delta_case(oracle, name)
            maps = _maps(enc, s, case.n)
            for g, mp in enumerate(maps):  # +inf exactly where the move leaves the alphabet - on the last grid too, whose
                # feature reads no source, and on every grid that is a source
                assert mp.dtype == np.float32 and mp.shape == (2,) + case.hw[g]
                assert np.array_equal(np.isinf(mp[0]), case.latents[g] == -64) and np.array_equal(np.isinf(mp[1]), case.latents[g] == 63), (name, g)
                assert not np.isnan(mp).any() and not (mp == -np.inf).any(), (name, g)
            worst = _check(case, maps, checks, "crafted layouts")
            n_big = max(case.n_dep(m, y, x) for m, y, x, _, _ in checks)
            print(f"{name}: {len(checks)} (position, sign) pairs, {case.n_decodes} oracle decodes, up to {n_big} dependents, "
                  f"worst deviation {worst:.3g} of the bound")
    finally:
        enc.close()


@pytest.mark.gpu
def test_rate_deltas_on_crafted_layouts(gpu, oracle):
    geo = [al.case(n).arch for n in DELTA_NAMES]
    assert any(a.total_context_arm % 2 and a.total_context_arm > 1 for a in geo) and any(a.n_hidden_layers_arm == 0 for a in geo)
    assert {al.case(n).placement for n in DELTA_NAMES if al.case(n).kind == "placement"} == set(PLACEMENT_FEATURES)
    assert sum(al.case(n).kind == "tiny" for n in DELTA_NAMES) == 2
    _check_deltas(gpu, oracle, DELTA_NAMES)


@pytest.mark.gpu
def test_rate_deltas_with_71_arm_inputs(gpu, oracle):
    """The hipFuncSetAttribute branch of launch_encode_deltas.  (The oracle's 221 decodes of a 71-input, 7-layer ARM are
    what this test's time goes to.)"""
    assert al.case("arm_s40_i31_h7").arch.total_context_arm == 71
    _check_deltas(gpu, oracle, ["arm_s40_i31_h7"])


# ---- the decoder ---------------------------------------------------------------------------------------------------------
def _feature_peak(oracle, c):
    """Largest |IFCE feature| the oracle computed for a case (a feature of 2^feat_bits or more is a sentinel in the pipelined
    entropy kernel's feature plane; the pixels that read it are redone in int64)."""
    return max([int(np.abs(f).max()) for f in al.entropy(oracle, c)["ctx_ifce"] if f is not None and f.size] + [0])


def _decode_and_check(oracle, cases, planes, **opts):
    """Every case the decoder takes in one DecodeBatch: latents = what was encoded, integer planes = oracle.decode_video's;
    returns [(case, kernel bits, pixels redone)] per slot."""
    from cool_chic_amd import DecodeBatch
    from cool_chic_amd._lib import CcdError

    b = DecodeBatch(0, **opts)
    try:
        for c in [c for c in cases if not al.device_decodable(c.arch)]:  # refused when added: an error, never another path
            with pytest.raises(CcdError) as e:
                b.add(c.hdr, c.nn, c.payload, 8, 0)
            assert e.value.code == ERR_UNSUPPORTED, c.name
        cases = [c for c in cases if al.device_decodable(c.arch)]
        for s, c in enumerate(cases):
            assert b.add(c.hdr, c.nn, c.payload, 8, 0) == s
        b.run()
        b.wait()
        out = []
        for s, c in enumerate(cases):
            assert b.slot_status(s) == 0, c.name
            for g, want in enumerate(c.latents):
                assert np.array_equal(b.latent(s, g), want), (c.name, g)
            if planes:
                for p, w in zip(b.planes(s), oracle.decode_video(c.stream)[0]["planes"]):
                    assert np.array_equal(p.astype(np.uint16), w), c.name
            out.append((c, b.slot_kernels(s), int(b.slot_stats(s)[39])))
        return out
    finally:
        b.close()


@pytest.mark.gpu
def test_crafted_layouts_through_the_decoder(gpu, oracle):
    """Production path.  The kernel is the one ccd_network_kernel_class names: pipelined below 64 ARM inputs (its instantiation
    with the device check of the features where the network's worst case asks for it), generic from 64 on."""
    from cool_chic_amd._lib import lib

    got = _decode_and_check(oracle, al.cases(), planes=True)
    assert len(got) == len(al.cases()) - 2
    n_redone = 0
    for c, k, n_redo in got:
        cls = lib().ccd_network_kernel_class(c.hdr, len(c.hdr), c.nn, len(c.nn))
        assert bool(k & 1) == bool(cls & 1) == (c.arch.total_context_arm < 64), (c.name, k, cls)
        if k & 1:
            assert bool(k & 16) == bool(cls & 16), (c.name, k, cls)
            peak = _feature_peak(oracle, c)
            assert (n_redo > 0) == (peak >= 1 << 15), (c.name, n_redo, peak)
            n_redone += n_redo
    print("pixels redone in int64 on the production path:", n_redone)


def _placement_cases():
    return [c for c in al.cases() if c.kind == "placement"] + [c for c in al.cases() if c.kind == "tiny" and c.placement]


@pytest.mark.gpu
def test_ifce_placements_through_the_feature_redo(gpu, oracle):
    """The sweep's "dyn9" variant (CCD_OPT_RANGE_BITS = 9) on the IFCE placements: features of 2^9 and more are sentinels, on the
    coarse raster-order grids and the hyperlatent grids too, and their pixels go through the int64 redo."""
    cases = _placement_cases()
    got = _decode_and_check(oracle, cases, planes=False, range_bits=9)
    coarse_only = 0
    for c, k, n_redo in got:
        assert k & 17 == 17, (c.name, k)
        peak = _feature_peak(oracle, c)
        assert (n_redo > 0) == (peak >= 1 << 9), (c.name, n_redo, peak)
        coarse_only += n_redo > 0 and c.placement in ((3, 15), (4, 4))
    assert coarse_only >= 4


@pytest.mark.gpu
def test_ifce_placements_on_the_generic_kernel(gpu, oracle, monkeypatch):
    monkeypatch.setenv("CCD_FORCE_GENERIC", "1")
    cases = _placement_cases()
    for c, k, _ in _decode_and_check(oracle, cases, planes=True):
        assert not k & 1, (c.name, k)
