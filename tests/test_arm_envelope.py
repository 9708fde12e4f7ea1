"""The integer-width envelope of the entropy stage at its own thresholds ("The integer-width envelope"; the
cases: tests/arm_envelope.py, the reference in Python integers: tests/arm_envelope_ref.py).

The reference's ARM and IFCE are wrapping int64 for any weights and data; the device keeps that with several evaluations, and
a handful of host inequalities choose among them.  CPU half: the restated classification equals the library's on every case
and on both sides of every weight and bound threshold, the restated forward equals the oracle on every case and on two trained
networks, every case really reaches what it is there for (census).  GPU half: all cases in one DecodeBatch, in a second one
with the matrix cores on and in a third forced to the generic kernel, against the encoded latents, the oracle's planes, the
predicted kernel bits and the predicted redo counts."""
import numpy as np
import pytest

import arm_envelope as ae
import arm_envelope_ref as ref
from conftest import load_arm_sweep, load_golden

NAMES = ae.NAMES
BIT_PIPE, BIT_MFMA, BIT_DYN = 1, 8, 16  # ccd_batch_slot_kernels; ccd_network_kernel_class has 1 and 16 and the flags from bit 16 up
T8 = 25  # ccd_entropy_pipe.hip: a grid whose widest wavefront step holds this many pixels runs 8-pixel tasks (the matrix cores' only ones)


def _library_flags(hdr, nn):
    from cool_chic_amd._lib import lib

    k = lib().ccd_network_kernel_class(hdr, len(hdr), nn, len(nn))
    assert k >= 0
    bit = lambda i: bool(k >> i & 1)
    assert lib().ccd_network_fits_fast_path(hdr, len(hdr), nn, len(nn)) == (k & 1)
    return dict(pipe=bit(0), dyn_bit=bit(4), narrow=bit(16), ifce_w32=bit(17), mfma=bit(18), w32=bit(19), dyn_act=bit(20), feat_i32=bit(21),
                dyn_feat=bit(22))


def _compare_flags(arch, ints, hdr, nn, what):
    fl = ref.classify(arch, ints)
    got = _library_flags(hdr, nn)
    want = dict(pipe=fl.pipe, dyn_bit=fl.pipe and fl.dyn_feat, narrow=fl.narrow, ifce_w32=fl.ifce_w32, mfma=fl.mfma, w32=fl.w32,
                dyn_act=fl.dyn_act, feat_i32=fl.feat_i32, dyn_feat=fl.dyn_feat)
    assert got == want, (what, got, want)
    return fl


def _wrap32(v):
    return ((int(v) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _check_forward(arch, f, r, what):
    """A restated forward against the oracle's table indices (decode order) and features (its int32 view)."""
    for g in range(arch.n_grids):
        assert np.array_equal(ref.in_decode_order(f.idx[g]), r["mu_scale_idx"][g]), (what, g)
        if r["ctx_ifce"][g] is not None:
            mine = np.array([_wrap32(v) for v in f.features[g].ravel()], dtype=np.int64).reshape(f.features[g].shape)
            assert np.array_equal(mine, r["ctx_ifce"][g]), (what, g)
    return f


# ---- CPU -------------------------------------------------------------------------------------------------------------
def test_signed_digits_end_below_the_bit_width():
    """What the matrix-core limits rest on: three signed-digit bytes hold -0x808080 .. 0x7F7F7F and two hold -0x8080 .. 0x7F7F;
    one more and the top digit is lost - 0x7F7F80 is inside 23 bits and outside three digits."""
    for n, lo, hi in ((3, -0x808080, ref.DIGITS3_MAX), (2, -0x8080, ref.DIGITS2_MAX)):
        for v in (lo, lo + 1, -1, 0, 1, hi - 1, hi):
            assert sum(d << (8 * j) for j, d in enumerate(ref.signed_digits(v, n))) == v, (n, v)
        for v in (lo - 1, hi + 1, (1 << (8 * n - 1)) - 1):
            assert sum(d << (8 * j) for j, d in enumerate(ref.signed_digits(v, n))) != v, (n, v)


@pytest.mark.parametrize("name", NAMES)
def test_every_case_sets_the_flags_it_is_there_for(name):
    """Restated flags = the library's (ccd_network_kernel_class, ccd_network_fits_fast_path) = the ones the case list names."""
    c = ae.case(name)
    fl = _compare_flags(c.arch, c.ints, c.hdr, c.nn, name)
    assert ae.Want(fl.w32, fl.dyn_act, fl.dyn_feat, fl.feat_i32, fl.ifce_w32, fl.narrow, fl.mfma) == c.want, name


def test_cases_differ_from_the_base_in_the_intended_flags_only():
    base = ae.case("base").want
    differ = {n: {f for f in base._fields if getattr(ae.case(n).want, f) != getattr(base, f)} for n in NAMES}
    assert differ["w32_under"] == {"mfma"} and differ["w32_plus"] == {"w32", "dyn_act", "narrow", "mfma"}  # (dyn_act is defined as set without w32)
    assert differ["act_under"] == set() and differ["act_over"] == {"dyn_act", "narrow", "mfma"}
    assert differ["feat_static"] == {"mfma"} and differ["feat_dyn"] == {"dyn_feat", "narrow", "mfma"}
    assert {f for f in base._fields if getattr(ae.case("feat_generic").want, f) != getattr(ae.case("feat_side_plane").want, f)} == {"feat_i32"}
    assert {f for f in base._fields if getattr(ae.case("ifce_w_over").want, f) != getattr(ae.case("ifce_w_under").want, f)} == {"ifce_w32"}
    assert {f for f in base._fields if getattr(ae.case("w32_minus_nohidden").want, f) != getattr(ae.case("w32_under_nohidden").want, f)} == {"w32", "dyn_act", "narrow"}
    for n in ("mf_edge_in", "mf_act_band", "mf_quiet", "mf_feat_max"):
        assert differ[n] == set(), n
    for n in ("mf_w_7f7f80", "mf_w_7fffff", "mf_w_2p23", "mf_feat_band"):  # inside `narrow`, outside the signed digits
        assert differ[n] == {"mfma"}, n


def _classified(net):
    from cool_chic_amd import writer
    from cool_chic_amd._lib import CCHeader

    a = CCHeader.from_buffer_copy(bytes(net.arch))
    nn = writer.encode_network(a, net.v.astype(np.int32))
    hdr = writer.cc_header_bytes(a)
    return _compare_flags(writer.parse_cc_header(hdr), net.v, hdr, nn, "threshold")


def test_both_sides_of_every_threshold():
    """One step below, on and one step above every limit of the table, classified by the library and by the restatement: an
    off-by-one in an inequality fails here without a stream being decoded.  The IFCE columns of the stabiliser take any integer
    as a weight (step 1), the other ARM weights and the IFCE weights multiples of 256; a feature of the last grid is its bias
    and its bound |bias| + 1."""
    lim = 1 << 31
    flat = ae.base_net(8, 4, 0, ae.SMALL, 101)  # no hidden layer: nothing but the overwritten weight moves a flag
    col = flat.stab_w(1, flat.n_sp + 2)
    for v, want in ((lim - 2, True), (lim - 1, True), (-(lim - 2), True), (-(lim - 1), True), (-lim, False)):
        net = ae.Net(flat.arch, flat.v)
        net.v[col] = v
        fl = _classified(net)
        assert fl.w32 == want and fl.max_abs_weight == abs(v) and fl.pipe == want, v
    for v, want in (((1 << 23) - 2, True), ((1 << 23) - 1, True), (1 << 23, False), ((1 << 23) + 1, False), (-(1 << 23), False)):
        net = ae.Net(flat.arch, flat.v)
        net.v[net.out_w(0, 1)] = v  # << 8
        assert _classified(net).w32 == want, v
        net = ae.Net(flat.arch, flat.v)
        net.quiet_ifce()
        net.v[net.ifce_w(1, 0, 0)] = v
        fl = _classified(net)
        assert fl.ifce_w32 == want and fl.feat_i32 and fl.w32 and fl.pipe, v
    deep = ae.base_net(8, 4, 2, ae.SMALL, 113)
    last = deep.arch.n_grids - 1
    # worst-case feature: 2^15 (the checking instantiation), 2^30 (the generic kernel), 0x7F7F + 1 (the matrix cores)
    for bound, flag in ((1 << 15, "dyn_feat"), (1 << 30, "feat_i32"), (ref.DIGITS2_MAX + 2, "mfma")):
        for b, beyond in ((bound - 2, False), (bound - 1, True), (bound, True), (-(bound - 2), False), (-(bound - 1), True)):
            net = ae.Net(flat.arch if flag == "feat_i32" else deep.arch, flat.v if flag == "feat_i32" else deep.v)
            net.quiet_ifce()
            net.v[net.ifce_b(last, 3)] = b
            fl = _classified(net)
            assert fl.worst_feature == abs(b) + 1
            assert getattr(fl, flag) == (beyond if flag == "dyn_feat" else not beyond), (flag, b)
    # matrix cores: the largest weight, in a column that takes any integer
    for v, want in ((ref.DIGITS3_MAX - 1, True), (ref.DIGITS3_MAX, True), (ref.DIGITS3_MAX + 1, False), ((1 << 23) - 1, False), (1 << 23, False),
                    (-ref.DIGITS3_MAX, True), (-ref.DIGITS3_MAX - 1, False)):
        net = ae.Net(deep.arch, deep.v)
        ae._mf_weights(5, v)(net)
        fl = _classified(net)
        assert fl.mfma == want and fl.narrow and fl.max_abs_weight == abs(v), v
    # dyn_act: the two values arm_envelope.largest_quiet_value separates
    v = ae.largest_quiet_value(deep)
    for dv, want in ((-1, False), (0, False), (1, True), (2, True)):
        net = ae.Net(deep.arch, deep.v)
        ae._unit_from_all_inputs(net, 5, -(v + dv))
        assert _classified(net).dyn_act == want, dv


@pytest.mark.parametrize("name", NAMES)
def test_forward_equals_the_oracle_and_the_stream_round_trips(oracle, name):
    c = ae.case(name)
    r = ae.entropy(oracle, c)
    assert r["n_symbols"] == c.arch.n_symbols
    assert np.array_equal(r["nn_ints"][:len(c.ints)], c.ints), name  # the payload carried the overwritten integers
    for g, (got, want) in enumerate(zip(r["latent"], c.latents)):  # the host writer's stream decodes to what was encoded
        assert np.array_equal(got, want), (name, g)
    _check_forward(c.arch, ae.forward(c), r, name)


def test_forward_equals_the_oracle_on_trained_networks(oracle):
    """The restatement pinned to the reference encoder's rgb192 and to one stream of the ARM sweep."""
    from cool_chic_amd import writer

    bs, _, _ = load_golden("rgb192")
    streams = {"rgb192": bs, "d12_h2_i2": load_arm_sweep()["d12_h2_i2"][0]}
    for name, stream in streams.items():
        hdr, nn, lat = oracle.split_stream(stream)[1][0][1][0]
        r = oracle.decode_coolchic(hdr, nn, lat, stop_after_entropy=True)
        arch = writer.parse_cc_header(hdr)
        f = _check_forward(arch, ref.forward(arch, r["nn_ints"], r["latent"]), r, name)
        assert f.census.n_wrapped == 0 and f.wide_pixels == 0
        _compare_flags(arch, r["nn_ints"], hdr, nn, name)


def _peaks(f, g=None):
    grids = range(len(f.peaks)) if g is None else [g]
    return np.array([int(v) for k in grids for v in f.peaks[k].ravel()], dtype=object)


def _features(f):
    return [int(v) for p in f.features if p is not None for v in p.ravel()]


def widest_step(h, w):
    if w <= 9:
        return 1
    return max(np.bincount([x + 10 * y for y in range(h) for x in range(w)]))


def coverage(case, forward):
    """Every condition the case list is there for, from the census (`case`, `forward`: name -> Case / Forward): a later change
    to the builders cannot lose a case silently."""
    lim = ref.LIM32
    cen = {n: forward(n).census for n in NAMES}
    # w32: the largest representable weight below 2^31, and 2^31 with either sign
    assert cen["w32_under"].max_abs_weight == cen["w32_under_nohidden"].max_abs_weight == (1 << 31) - 256
    assert cen["w32_plus"].max_abs_weight == cen["w32_minus_nohidden"].max_abs_weight == 1 << 31
    assert min(case("w32_minus_nohidden").ints) == -(1 << 23) and max(case("w32_plus").ints) == 1 << 23
    assert case("w32_minus_nohidden").arch.n_hidden_layers_arm == 0
    # dyn_act: a real activation within a factor 2 of int32's end, on either side of the bound
    assert lim // 2 < cen["act_under"].max_activation <= lim, cen["act_under"]
    assert lim // 2 < cen["act_over"].max_activation and cen["base"].max_activation < lim // 256
    # dyn_feat: the static side reaches 2^15 - 2 and no further; the checking side passes 2^15 with the four edge values
    assert cen["feat_static"].max_feature == 32766 and forward("feat_static").wide_pixels == 0
    seen = set(_features(forward("feat_dyn")))
    assert {32767, 32768, -32768, -32769} <= seen, "the four features around the int16 plane's sentinel"
    assert forward("feat_dyn").wide_pixels > 1000 and max(seen) > 36000 and min(seen) < -36000
    assert any(widest_step(case("feat_dyn").arch.grid_h[g], case("feat_dyn").arch.grid_w[g]) >= T8 for g in range(3))
    # feat_i32: a real feature above 2^29 that float32 rounds, in the side plane / a feature of 2^30
    side = _features(forward("feat_side_plane"))
    assert (1 << 29) < max(side) < (1 << 30) and any(int(np.float32(v)) != v for v in range(max(side) - 200, max(side) + 200))
    assert cen["feat_generic"].max_feature >= 1 << 30
    # ifce_w32: a real feature of 2^29 from a weight of 2^31, and from the largest weight below
    assert cen["ifce_w_over"].max_feature == 1 << 29 and (1 << 28) < cen["ifce_w_under"].max_feature < 1 << 29
    assert forward("ifce_w_over").wide_pixels > 100 and forward("ifce_w_under").wide_pixels > 100
    # narrow: beyond int32 without a wrap / with sums that leave int64 and change table indices
    assert cen["narrow_big"].max_abs_weight == 1 << 31 and cen["narrow_big"].n_wrapped == 0 and cen["narrow_big"].max_activation > lim
    assert cen["narrow_wrap"].n_wrapped > 100, cen["narrow_wrap"]
    c = case("narrow_wrap")
    unwrapped = ref.forward(c.arch, c.ints, c.latents, wrap=False)
    assert any((a != b).any() for a, b in zip(unwrapped.idx, forward("narrow_wrap").idx)), "the wrap changes no table index"
    assert case("narrow_generic").arch.total_context_arm == 65 and cen["narrow_generic"].n_wrapped == 0
    # matrix cores: weights on both sides of three digits, activations inside 0x7F7F80 .. 0x7FFFFF and from 2^23 on, features
    # inside 32 640 .. 32 767, and a network that meets none of it
    d3, d2 = ref.DIGITS3_MAX, ref.DIGITS2_MAX
    assert [cen[n].max_abs_weight for n in ("mf_edge_in", "mf_act_band", "mf_quiet", "mf_w_7f7f80", "mf_w_7fffff", "mf_w_2p23")] == \
        [d3, d3, d3, d3 + 1, (1 << 23) - 1, 1 << 23]
    assert -((1 << 23) - 1) in case("mf_w_7fffff").ints and -d3 in case("mf_w_7f7f80").ints
    band = lambda p: ((p > d3) & (p < 1 << 23)).sum()
    p0 = _peaks(forward("mf_edge_in"), 0)
    assert band(p0) > 1000 and (p0 >= 1 << 23).sum() > 1000 and (p0 <= d3).sum() > 1000
    p0 = _peaks(forward("mf_act_band"), 0)
    assert band(p0) == p0.size and cen["mf_act_band"].max_activation == 0x7FFF80
    assert cen["mf_quiet"].max_activation == d3
    for n in ("mf_feat_max", "mf_feat_band"):
        assert cen[n].max_activation < d3 // 1.5, n  # no redo hides what the features do
    assert cen["mf_feat_max"].max_feature == d2 and 32766 >= cen["mf_feat_band"].max_feature > d2 + 100
    assert sum(1 for v in _features(forward("mf_feat_band")) if v > d2) > 10000
    for n in NAMES:  # the matrix cores serve 8-pixel tasks only: the cases that must reach them are wide enough
        a = case(n).arch
        if n.startswith("mf_") and case(n).want.mfma:
            assert widest_step(a.grid_h[0], a.grid_w[0]) >= T8, n
        if case(n).want.mfma and widest_step(a.grid_h[0], a.grid_w[0]) >= T8:
            # what test_matrix_core_cases predicts the redo counter from: all over the grid or nowhere, never a few pixels
            # that could all sit in the 4- and 2-pixel tasks of the grid's first and last steps
            over = int((_peaks(forward(n), 0) > d3).sum())
            assert over == 0 or over > 500, (n, over)


def test_coverage():
    coverage(ae.case, lambda n: ae.forward(ae.case(n)))


def _moved(name, **damage):
    """Pixels whose table indices move when every ARM weight / hidden activation / feature passes through a too narrow form."""
    c = ae.case(name)
    bad = ref.forward(c.arch, c.ints, c.latents, damage=damage)
    return sum(int((a != b).any(axis=2).sum()) for a, b in zip(ae.forward(c).idx, bad.idx))


def test_every_case_can_tell():
    """Reaching a value is not enough: a network whose outputs sit at the ends of the tables decodes the same whatever the ARM
    computes.  For every hazard the restated forward is run once more with the representation error a too narrow evaluation
    would make; the case it belongs to must move table indices at many pixels, the case on the other side at none."""
    int16_or_sentinel = lambda v: -32768 if (v >= 1 << 15 or v <= -(1 << 15)) else v
    hazards = [  # (case that must move, case that must not, what is damaged, how)
        ("w32_plus", "w32_under", "weight", ref.keep_bits(32)), ("w32_minus_nohidden", "w32_under_nohidden", "weight", ref.keep_bits(32)),  # (-2^31: the limit is on the magnitude, int32 holds it)
        ("narrow_big", "base", "weight", ref.keep_bits(32)), ("narrow_wrap", "base", "weight", ref.keep_bits(32)),
        ("act_over", "act_under", "activation", ref.keep_bits(32)),  # (over: the bound; its real activations stay inside too)
        ("feat_dyn", "feat_static", "feature", ref.keep_bits(16)), ("feat_dyn", "feat_static", "feature", int16_or_sentinel),
        ("feat_side_plane", "base", "feature", ref.keep_bits(16)), ("feat_side_plane", "base", "feature", int16_or_sentinel),
        ("feat_generic", "base", "feature", int16_or_sentinel),
        ("ifce_w_over", "base", "feature", int16_or_sentinel), ("ifce_w_under", "base", "feature", int16_or_sentinel),
        ("mf_w_7fffff", "mf_quiet", "weight", ref.keep_digits(3)), ("mf_w_7f7f80", "mf_quiet", "weight", ref.keep_digits(3)),
        ("mf_w_2p23", "mf_quiet", "weight", ref.keep_digits(3)),
        ("mf_act_band", "mf_quiet", "activation", ref.keep_digits(3)), ("mf_edge_in", "mf_quiet", "activation", ref.keep_digits(3)),
        ("mf_feat_band", "mf_feat_max", "feature", ref.keep_digits(2)),
    ]
    for moves, stays, what, how in hazards:
        n = _moved(moves, **{what: how})
        assert _moved(stays, **{what: how}) == 0, (stays, what)
        if moves in ("act_over", "w32_minus_nohidden"):
            assert n == 0  # act_over: the worst case is a bound, no latents reach it from V + 1 (act_under comes within 0.07 % of it)
        else:
            assert n > 50, (moves, what, n)
    assert _moved("act_under", activation=ref.keep_bits(31)) > 100  # one bit less than the pipelined kernel's operand: 248 pixels
    # the float32 round trip of a feature above 2^24 is visible in feat_side_plane
    c = ae.case("feat_side_plane")
    keep, ref._float32_round_trip = ref._float32_round_trip, int
    try:
        exact = ref.forward(c.arch, c.ints, c.latents)
    finally:
        ref._float32_round_trip = keep
    assert sum(int((a != b).any(axis=2).sum()) for a, b in zip(ae.forward(c).idx, exact.idx)) > 50


# ---- GPU -------------------------------------------------------------------------------------------------------------
def _decode_all(oracle, planes, **opts):
    """Every case in ONE DecodeBatch (the instantiations fork and join as in production): status, latents = what was encoded,
    integer planes = oracle.decode_video's; returns {name: (kernel bits, redo counter)}."""
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cool_chic_amd import DecodeBatch

    cases = ae.cases()
    b = DecodeBatch(0, **opts)
    try:
        for s, c in enumerate(cases):
            assert b.add(c.hdr, c.nn, c.payload, 8, 0) == s
        b.run()
        b.wait()
        out = {}
        for s, c in enumerate(cases):
            assert b.slot_status(s) == 0, c.name
            for g, want in enumerate(c.latents):
                assert np.array_equal(b.latent(s, g), want), (c.name, g, b.slot_kernels(s))
            if planes:
                for p, w in zip(b.planes(s), oracle.decode_video(c.stream)[0]["planes"]):
                    assert np.array_equal(p.astype(np.uint16), w), c.name
            out[c.name] = (b.slot_kernels(s), int(b.slot_stats(s)[39]))
        return out
    finally:
        b.close()


def _flags(c):
    return ref.classify(c.arch, c.ints)


@pytest.mark.gpu
def test_every_case_on_the_production_path(oracle):
    """The kernel is the one the restated classification predicts; the checking instantiation redoes exactly the pixels that
    read a wide feature (ccd_entropy_pipe.hip counts pixels there), the static one none."""
    got = _decode_all(oracle, planes=True)
    n_generic = 0
    for c in ae.cases():
        k, n_redo = got[c.name]
        fl = _flags(c)
        assert bool(k & BIT_PIPE) == fl.pipe and not k & BIT_MFMA, (c.name, k)
        n_generic += not fl.pipe
        if fl.pipe:
            assert bool(k & BIT_DYN) == fl.dyn_feat, (c.name, k)
            assert n_redo == (ae.forward(c).wide_pixels if fl.dyn_feat else 0), (c.name, n_redo, ae.forward(c).wide_pixels)
    assert n_generic >= 7


@pytest.mark.gpu
def test_matrix_core_cases(oracle):
    """The same batch with CCD_OPT_MFMA_ARM = 1: the matrix cores take exactly the networks inside the signed digits; a task that
    holds an activation above 0x7F7F7F is redone (the counter counts tasks there), the others are not."""
    got = _decode_all(oracle, planes=False, mfma_arm=1)
    on_cores = []
    for c in ae.cases():
        k, n_redo = got[c.name]
        fl = _flags(c)
        assert bool(k & BIT_PIPE) == fl.pipe and bool(k & BIT_MFMA) == fl.mfma, (c.name, k)
        if fl.mfma:
            assert not k & BIT_DYN
            a = c.arch
            over = sum(int((_peaks(ae.forward(c), g) > ref.DIGITS3_MAX).sum()) for g in range(a.n_grids) if widest_step(a.grid_h[g], a.grid_w[g]) >= T8)
            assert (n_redo > 0) == (over > 0), (c.name, n_redo, over)
            on_cores.append(c.name)
        elif fl.pipe:
            assert bool(k & BIT_DYN) == fl.dyn_feat and n_redo == (ae.forward(c).wide_pixels if fl.dyn_feat else 0), (c.name, k, n_redo)
    assert {"mf_edge_in", "mf_act_band", "mf_quiet", "mf_feat_max"} <= set(on_cores)


@pytest.mark.gpu
def test_every_case_forced_to_the_generic_kernel(oracle, monkeypatch):
    """CCD_FORCE_GENERIC: the generic cases give what they gave without it, the pipelined ones the same latents and planes."""
    monkeypatch.setenv("CCD_FORCE_GENERIC", "1")
    for name, (k, _) in _decode_all(oracle, planes=True).items():
        assert not k & BIT_PIPE, (name, k)
