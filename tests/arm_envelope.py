"""Cool-chics whose ARM / IFCE integers sit on both sides of every threshold that selects an evaluation of the integer ARM on
the device ("The integer-width envelope"): int32 weights, int32 activations, 16-bit and 30-bit features,
int32 IFCE weights, the non-wrapping envelope `narrow`, and the signed-digit limits of the matrix-core path.  Built like
arm_layouts.build_stream: architecture derived from the reference-encoded `rgb192` fixture, a network drawn from its trained
values, a few integers overwritten, the host writer for the stream.  Every case is made once per process; the yardsticks are
tests/arm_envelope_ref.py (Python integers), the CPU oracle and the host writer.

Quantisation steps: ARM weights 2^-8 (fixed point = integer << 8, the IFCE columns of the first layer and of the stabiliser
<< 0: any integer is a weight there), IFCE weights and biases 2^-8 (so a feature is exactly bias + sum weight x latent)."""
from collections import namedtuple

import numpy as np

import arm_envelope_ref as ref
import arm_layouts as al

Q_ARM_W, Q_IFCE = -8, -8
SMALL, WIDE = (18, 65), (32, 320)
# the flags a case is there for (Flags of arm_envelope_ref.classify); test_every_case_sets_the_flags_it_is_there_for compares all
Want = namedtuple("Want", "w32 dyn_act dyn_feat feat_i32 ifce_w32 narrow mfma")
Case = namedtuple("Case", "name arch ints hdr nn payload cc stream latents want")

_CASES = {}
_FORWARD = {}
_ENTROPY = {}


class Net:
    """The transmitted integers of one cool-chic (int64) with the positions of the ARM and IFCE parameters by name."""

    def __init__(self, arch, ints):
        from cool_chic_amd import writer

        self.arch, self.v = arch, np.array(ints, dtype=np.int64)
        self.dim, self.nh, self.n_if = arch.total_context_arm, arch.n_hidden_layers_arm, arch.output_feature_ifce
        self.n_sp = arch.spatial_context_arm
        self.n = writer.network_layout(arch)
        self.fin = [int(arch.input_features_ifce[g]) for g in range(arch.n_grids)]
        assert arch.linear_stabiliser_arm

    def hidden_w(self, layer, out, inp):
        return layer * self.dim * self.dim + out * self.dim + inp

    def out_w(self, out, inp):
        return self.nh * self.dim * self.dim + out * self.dim + inp

    def stab_w(self, out, inp):
        return self.nh * self.dim * self.dim + 2 * self.dim + out * self.dim + inp

    def hidden_b(self, layer, out):
        return self.n[0] + layer * self.dim + out

    def out_b(self, out):
        return self.n[0] + self.nh * self.dim + out

    def ifce_w(self, g, out, chan):
        assert self.fin[g] > chan
        return self.n[0] + self.n[1] + sum(self.n_if * f for f in self.fin[:g]) + out * self.fin[g] + chan

    def ifce_b(self, g, out):
        assert self.fin[g] > 0
        return self.n[0] + self.n[1] + self.n[2] + self.n_if * sum(f > 0 for f in self.fin[:g]) + out

    def quiet_ifce(self):
        """Every IFCE parameter 0: the features are what a case then writes."""
        self.v[self.n[0] + self.n[1]:sum(self.n[:4])] = 0


def base_net(n_sp, n_if, n_hidden, size, seed):
    """Drawn like arm_layouts.draw_network, IFCE on every grid, re-expressed at this module's quantisation steps (the same
    fixed-point network), the IFCE a quarter of the drawn one so that its worst case stays below 2^15."""
    from cool_chic_amd import writer

    donor, donor_ints, _ = al.donor()
    q = [int(x) for x in donor.nn_q_step_log2]
    new_q = list(q)
    new_q[0], new_q[2], new_q[3] = Q_ARM_W, Q_IFCE, Q_IFCE
    changes = dict(spatial_context_arm=n_sp, n_hidden_layers_arm=n_hidden, output_feature_ifce=n_if, img_size=tuple(size),
                   nn_q_step_log2=tuple(new_q))
    changes.update(dict(has_ifce_resolution=1, ifce_resolution=(0, 15)) if n_if else dict(has_ifce_resolution=0))
    arch = writer.derive_arch(donor, **changes)
    ints = al.draw_network(donor, donor_ints, arch, np.random.default_rng(seed)).astype(np.int64)
    n = writer.network_layout(arch)
    at = np.cumsum([0] + n)
    for k, gain in ((0, 1.0), (2, 0.25), (3, 0.25)):
        ints[at[k]:at[k + 1]] = np.round(ints[at[k]:at[k + 1]] * gain * 2.0 ** (q[k] - new_q[k])).astype(np.int64)
    return Net(arch, ints)


def minus64_block(lat, g=0):
    """A patch of -64 larger than the context window in grid g: pixels inside see -64 in every spatial context."""
    a = lat[g]
    a[4:14, 20:45] = -64
    return lat


# ---- the overwrites: one function per case, (Net) -> None, and the latents -----------------------------------------------
def _unit_from_all_inputs(net, unit, value, layer=0):
    """Hidden unit `unit` reads every spatial context with `value`, no feature, no bias; the next layer reads it with 1 / -1."""
    for i in range(net.dim):
        net.v[net.hidden_w(layer, unit, i)] = value if i < net.n_sp else 0
    net.v[net.hidden_b(layer, unit)] = 0
    for o in range(net.dim if layer + 1 < net.nh else 2):
        at = net.hidden_w(layer + 1, o, unit) if layer + 1 < net.nh else net.out_w(o, unit)
        net.v[at] = 1 if o % 2 else -1


def largest_quiet_value(net, unit=5):
    """The largest V for which a hidden unit reading every spatial context with -V keeps the worst-case activation inside int32
    (found by bisection on the restated classification: V + 1 leaves it)."""
    lo, hi = 1, 1 << 22
    while hi - lo > 1:
        mid = (lo + hi) // 2
        trial = Net(net.arch, net.v)
        _unit_from_all_inputs(trial, unit, -mid)
        if ref.classify(trial.arch, trial.v).dyn_act:
            hi = mid
        else:
            lo = mid
    return lo


def _w_out(value, out, inp):
    def f(net):
        net.v[net.out_w(out, inp)] = value
    return f


def _w_stab(value, out, inp):
    def f(net):
        net.v[net.stab_w(out, inp)] = value
    return f


def _act(delta):
    def f(net):
        _unit_from_all_inputs(net, 5, -(largest_quiet_value(net) + delta))
    return f


def _last_grid_features(values):
    def f(net):
        g = net.arch.n_grids - 1
        for o, v in enumerate(values):
            net.v[net.ifce_b(g, o)] = v
            net.v[net.ifce_w(g, o, 0)] = 0
    return f


def _feat_static(net):
    """Worst case exactly 2^15 - 1: a feature of 32 766 on the last grid (bound = |bias| + 1), every other bound below."""
    _last_grid_features([32766, -32766, 5, -5])(net)


def _feat_dyn(net):
    """32 767, 32 768, -32 768 and -32 769 on the last grid; on grids 0 and 2 feature 0 = 600 x the next grid's latent: beyond
    +-2^15 where that latent is -64, 63 or 55 and more."""
    _last_grid_features([32767, 32768, -32768, -32769])(net)
    for g in (0, 2):
        net.v[net.ifce_w(g, 0, 0)] = 600
        net.v[net.ifce_b(g, 0)] = 0
        for c in range(1, net.fin[g]):
            net.v[net.ifce_w(g, 0, c)] = 0


def _feat_i32(bias):
    def f(net):
        """On grid 1 feature 1 = bias + 3 x the next grid's latent and feature 2 = bias; float32 rounds both (above 2^24).  The
        output layer reads them with 64 and -64: the difference moves mu by 16 table indices per float32 step, so the outputs
        stay inside the tables and tell a feature that lost its upper bits (or its rounding) from the right one."""
        net.quiet_ifce()
        net.v[net.ifce_b(1, 1)] = net.v[net.ifce_b(1, 2)] = bias
        net.v[net.ifce_w(1, 1, 0)] = 3
        for o in range(2):
            net.v[net.out_w(o, net.n_sp + 1)], net.v[net.out_w(o, net.n_sp + 2)] = 64, -64
            net.v[net.stab_w(o, net.n_sp + 1)] = net.v[net.stab_w(o, net.n_sp + 2)] = 0
    return f


def _ifce_weight(value):
    def f(net):
        net.quiet_ifce()
        net.v[net.ifce_w(1, 0, 0)] = value
        net.v[net.ifce_b(0, 1)] = 7
    return f


def _narrow_big(net):
    net.v[net.hidden_w(0, 3, 2)] = 1 << 23


def _narrow_wrap(net):
    _unit_from_all_inputs(net, 5, -((1 << 31) - 1))


def _mf_features(net, f0_bias, f0_weight, others=(1, 0, 0)):
    """Feature 0 = f0_bias + f0_weight x the next grid's latent on every grid, features 1.. constant."""
    net.quiet_ifce()
    for g in range(net.arch.n_grids):
        net.v[net.ifce_b(g, 0)] = f0_bias
        net.v[net.ifce_w(g, 0, 0)] = f0_weight
        for o, v in enumerate(others[:net.n_if - 1]):
            net.v[net.ifce_b(g, 1 + o)] = v


def _mf_unit(net, unit, feature, weight, feature2=None, weight2=0):
    """Hidden unit `unit` of the first layer = ReLU(weight x feature [+ weight2 x feature2]): every other weight, the residual
    unit and the bias 0; the next layer reads it with +-2^-8, so that an activation of 128.0 moves the outputs without
    saturating them."""
    for i in range(net.dim):
        net.v[net.hidden_w(0, unit, i)] = 0
    net.v[net.hidden_w(0, unit, unit)] = -(1 << -Q_ARM_W)  # x 2^(16 + Q_ARM_W) = -(1 << 16): cancels the residual unit
    assert unit < net.n_sp
    net.v[net.hidden_w(0, unit, net.n_sp + feature)] = weight
    if feature2 is not None:
        net.v[net.hidden_w(0, unit, net.n_sp + feature2)] = weight2
    net.v[net.hidden_b(0, unit)] = 0
    for o in range(net.dim):
        net.v[net.hidden_w(1, o, unit)] = 1 if (o + unit) % 2 else -1


def _mf_weights(w, w_back):
    def f(net):
        """Features 1 and 2 = 1 everywhere.  Unit 2 = ReLU(w x feature 1 - (w - 2^16) x feature 2) = 1.0 and the stabiliser
        reads feature 1 with w and feature 2 with w_back (their sum: a few table indices): the largest weights of the network
        cancel, so the outputs stay inside the tables and a weight that lost a digit moves them."""
        _mf_features(net, 2, 0, others=(1, 1, 0))
        _mf_unit(net, 2, 1, w, 2, -(w - (1 << 16)))
        net.v[net.stab_w(0, net.n_sp + 1)] = w
        net.v[net.stab_w(0, net.n_sp + 2)] = w_back
    return f


def _mf_edge_in(net):
    """Weights of +-0x7F7F7F (the largest three signed digits hold); feature 0 = 2 + latent, unit 4 = ReLU(0x3FFFC0 x feature 0):
    0x7FFF80 (inside 0x7F7F80 .. 0x7FFFFF) where the latent is 0, 2^23 and more where it is positive."""
    _mf_weights(ref.DIGITS3_MAX, -ref.DIGITS3_MAX + 700)(net)
    for g in range(net.arch.n_grids):
        net.v[net.ifce_w(g, 0, 0)] = 1
    _mf_unit(net, 4, 0, 0x3FFFC0)


def _mf_act_band(net):
    """Feature 0 = 2 everywhere: unit 4 = 0x7FFF80 at every pixel, inside 0x7F7F80 .. 0x7FFFFF, and nothing reaches 2^23."""
    _mf_edge_in(net)
    for g in range(net.arch.n_grids):
        net.v[net.ifce_w(g, 0, 0)] = 0


def _mf_quiet(net):
    """The same network with feature 0 = 2, unit 4 = ReLU(0x3FBFBF x feature 0) = 0x7F7F7E and unit 6 = 0x7F7F7F; the drawn
    units stay far below."""
    _mf_weights(ref.DIGITS3_MAX, -ref.DIGITS3_MAX + 700)(net)
    _mf_unit(net, 4, 0, 0x3FBFBF)
    _mf_unit(net, 6, 1, ref.DIGITS3_MAX)  # 0x7F7F7F itself: the largest activation that is not redone


def _mf_feat(bias, weight):
    def f(net):
        """Feature 0 = bias + weight x latent; the hidden unit that would carry it on (x 2^8, the residual unit) reads it
        with a drawn weight like the other units do, so no activation leaves three digits because of it."""
        _mf_features(net, bias, weight, others=(0, 0, 0))
        net.v[net.hidden_w(0, net.n_sp, net.n_sp)] -= 1 << 8
    return f


T, F = True, False
# (name, picture, spatial contexts, IFCE features, hidden layers, seed, overwrite, -64 block?, the flags it is there for)
SPECS = [
    ("base", SMALL, 8, 4, 2, 100, None, F, Want(T, F, F, T, T, T, T)),
    # w32: the largest multiple of the weight's step below 2^31 / 2^31 itself, in the output layer and the stabiliser
    ("w32_under", SMALL, 8, 4, 2, 100, _w_out((1 << 23) - 1, 0, 3), F, Want(T, F, F, T, T, T, F)),
    ("w32_plus", SMALL, 8, 4, 2, 100, _w_stab(1 << 23, 1, 2), F, Want(F, T, F, T, T, F, F)),
    ("w32_under_nohidden", SMALL, 8, 4, 0, 101, _w_out(-((1 << 23) - 1), 0, 1), F, Want(T, F, F, T, T, T, F)),
    ("w32_minus_nohidden", SMALL, 8, 4, 0, 101, _w_out(-(1 << 23), 0, 1), F, Want(F, T, F, T, T, F, F)),
    # dyn_act: the worst-case hidden activation just inside / just outside int32, and latents that come within 2 of it
    ("act_under", SMALL, 8, 4, 2, 100, _act(0), T, Want(T, F, F, T, T, T, T)),
    ("act_over", SMALL, 8, 4, 2, 100, _act(1), T, Want(T, T, F, T, T, F, F)),
    # dyn_feat: worst case 2^15 - 1 / features that really pass 2^15
    ("feat_static", SMALL, 8, 4, 2, 100, _feat_static, F, Want(T, F, F, T, T, T, F)),
    ("feat_dyn", WIDE, 8, 4, 2, 102, _feat_dyn, F, Want(T, F, T, T, T, F, F)),
    # feat_i32: a feature above 2^29 in the int32 side plane / a worst case of 2^30
    ("feat_side_plane", SMALL, 8, 4, 0, 101, _feat_i32((3 << 28) + 0x8000 + 33), F, Want(T, F, T, T, T, F, F)),
    ("feat_generic", SMALL, 8, 4, 0, 101, _feat_i32((1 << 30) + 0x8000 + 33), F, Want(T, F, T, F, T, F, F)),
    # ifce_w32: an IFCE weight of 2^31 - 256 / 2^31, the worst-case feature below 2^30 either way
    ("ifce_w_under", SMALL, 8, 4, 0, 101, _ifce_weight((1 << 23) - 1), F, Want(T, F, T, T, T, F, F)),
    ("ifce_w_over", SMALL, 8, 4, 0, 101, _ifce_weight(1 << 23), F, Want(T, F, T, T, F, F, F)),
    # narrow: hidden weights beyond int32 whose sums stay below 2^62 / wrap int64
    ("narrow_big", SMALL, 8, 4, 2, 100, _narrow_big, F, Want(F, T, F, T, T, F, F)),
    ("narrow_wrap", SMALL, 8, 4, 2, 100, _narrow_wrap, T, Want(F, T, F, T, T, F, F)),
    # ... and the generic kernel's 32-bit form: 65 inputs, every bound inside `narrow`
    ("narrow_generic", SMALL, 40, 25, 1, 104, None, F, Want(T, F, F, T, T, T, F)),
    # matrix cores: the signed-digit limits of weights, activations and features
    ("mf_edge_in", WIDE, 8, 4, 2, 113, _mf_edge_in, F, Want(T, F, F, T, T, T, T)),
    ("mf_act_band", WIDE, 8, 4, 2, 113, _mf_act_band, F, Want(T, F, F, T, T, T, T)),
    ("mf_quiet", WIDE, 8, 4, 2, 113, _mf_quiet, F, Want(T, F, F, T, T, T, T)),
    ("mf_w_7f7f80", SMALL, 8, 4, 2, 113, _mf_weights(0x7F7F80, -0x7F7F7F), F, Want(T, F, F, T, T, T, F)),
    ("mf_w_7fffff", WIDE, 8, 4, 2, 113, _mf_weights(0x7FFFFF, -0x7FFFFF), F, Want(T, F, F, T, T, T, F)),
    ("mf_w_2p23", SMALL, 8, 4, 2, 113, _mf_weights(1 << 23, -(1 << 23) + 300), F, Want(T, F, F, T, T, T, F)),
    ("mf_feat_max", WIDE, 8, 4, 2, 113, _mf_feat(32575, -1), F, Want(T, F, F, T, T, T, T)),    # 32 639 where the latent is -64
    ("mf_feat_band", WIDE, 8, 4, 2, 113, _mf_feat(32702, 1), F, Want(T, F, F, T, T, T, F)),    # 32 638 .. 32 765, bound 2^15 - 1
]
NAMES = [s[0] for s in SPECS]


def build(spec, skip_overwrite=False):
    from cool_chic_amd import writer
    from oracle import oracle_py

    name, size, n_sp, n_if, n_hidden, seed, overwrite, block, want = spec
    net = base_net(n_sp, n_if, n_hidden, size, seed)
    if overwrite is not None and not skip_overwrite:
        overwrite(net)
    assert np.abs(net.v).max() < 1 << 31
    lat = al.extreme_latents(net.arch, seed + 1)
    if block:
        lat = minus64_block(lat)
    nn = writer.encode_network(net.arch, net.v.astype(np.int32))
    stream = writer.encode_stream(writer.cc_header_bytes(net.arch), nn, lat, bitdepth=8, frame_data_type=0)
    (_fh, ccs), = oracle_py.split_stream(stream)[1]
    hdr, nn, payload = ccs[0]
    lat = [np.ascontiguousarray(a, dtype=np.int8) for a in lat]
    return Case(name, writer.parse_cc_header(hdr), net.v, hdr, nn, payload, hdr + nn + payload, stream, lat, want)


def case(name):
    if name not in _CASES:
        _CASES[name] = build(next(s for s in SPECS if s[0] == name))
    return _CASES[name]


def cases():
    return [case(n) for n in NAMES]


def forward(c):
    """arm_envelope_ref.forward of a case, once."""
    if c.name not in _FORWARD:
        _FORWARD[c.name] = ref.forward(c.arch, c.ints, c.latents)
    return _FORWARD[c.name]


def entropy(oracle, c):
    if c.name not in _ENTROPY:
        _ENTROPY[c.name] = oracle.decode_coolchic(c.hdr, c.nn, c.payload, stop_after_entropy=True)
    return _ENTROPY[c.name]
