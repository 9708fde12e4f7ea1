"""The integer ARM and IFCE of a cool-chic restated in Python integers ("The integer-width envelope"):
fixed point (armint.py:30-170), forward over a whole latent pyramid (armint.py:180-203, arm.py:501-509, upsampling.py:582-588,
coolchic.py:89-146) and the host's classification of a network (ccd_format.cpp::decode_network / analyse_bounds).  It shares
no code with the library, the oracle or the writer: it takes a parsed header for the geometry, the transmitted integers and
the latents, and nothing else.

Every sum is formed in unbounded integers and reduced to signed 64 bits ONCE, before its arithmetic shift: that is where
torch's wrapping int64 and the integers part, and what the census counts.  Rows of a matrix product whose worst case
sum |x| |w| + |b| stays below 2^62 are evaluated in numpy int64 (exact there: no partial sum can leave int64), the others in
Python integers (object arrays)."""
from collections import namedtuple

import numpy as np

# arm.py:501-509: priority of each of the 40 causal positions of the 9 x 9 mask, row-major
PRIORITY = [38, 35, 30, 25, 23, 31, 36, 37, 39, 33, 28, 21, 20, 6, 15, 22, 29, 34, 32, 18, 12, 10, 5, 9, 14, 19, 27, 24, 13, 8, 2, 1,
            3, 11, 17, 26, 16, 7, 4, 0]
WEIGHT_SHIFT, FRAC_INTER = 16, 8  # constants.py:17,39
MU_OFFSET, N_MU, SCALE_OFFSET, N_SCALE = 16384, 32768, 1280, 2561
LIM32 = (1 << 31) - 1
DIGITS3_MAX, DIGITS2_MAX = 0x7F7F7F, 0x7F7F  # largest value of three / two signed-digit bytes (the matrix-core operands)

Fixed = namedtuple("Fixed", "w b ws bs")  # w[l]: object array [in][out], b[l]: [out]; ws [dim][outputs], bs [outputs] (zeros when absent)
Params = namedtuple("Params", "arm ifce")  # ifce[g]: Fixed of one layer, or None
Census = namedtuple("Census", "max_abs_weight max_activation max_feature n_wrapped n_sums")
Forward = namedtuple("Forward", "idx features wide_pixels peaks census")
Flags = namedtuple("Flags", "w32 dyn_act dyn_feat feat_i32 ifce_w32 narrow max_abs_weight worst_feature mfma pipe")


def wrap64(v):
    return ((int(v) + (1 << 63)) & ((1 << 64) - 1)) - (1 << 63)


def _wrap_array(a):
    out = np.empty(a.shape, dtype=object)
    flat, oflat = a.ravel(), out.ravel()
    for i in range(flat.size):
        oflat[i] = wrap64(flat[i])
    return out


def _obj(a):
    return np.asarray(a).astype(object)  # numpy integers become Python integers


# ---- the transmitted integers, by name -------------------------------------------------------------------------------
def split(arch, ints):
    """arm.w (hidden layers [out][in], output layer [2][in], stabiliser [2][in]), arm.b, ifce.w per grid with features [out][in],
    ifce.b: the first four groups of the stream (neuralnet.py:92-204)."""
    ints = [int(v) for v in ints]
    dim, nh, n_if = arch.total_context_arm, arch.n_hidden_layers_arm, arch.output_feature_ifce
    pos = 0

    def take(n):
        nonlocal pos
        pos += n
        return ints[pos - n:pos]

    outs = [dim] * nh + [2]
    w = [np.array(take(o * dim), dtype=object).reshape(o, dim) for o in outs]
    ws = np.array(take(2 * dim), dtype=object).reshape(2, dim) if arch.linear_stabiliser_arm else None
    b = [np.array(take(o), dtype=object) for o in outs]
    bs = np.array(take(2), dtype=object) if arch.linear_stabiliser_arm else None
    fin = [int(arch.input_features_ifce[g]) for g in range(arch.n_grids)]
    fw = [np.array(take(n_if * f), dtype=object).reshape(n_if, f) if f else None for f in fin]
    fb = [np.array(take(n_if), dtype=object) if f else None for f in fin]
    return dict(w=w, b=b, ws=ws, bs=bs, ifce_w=fw, ifce_b=fb)


# ---- fixed point -----------------------------------------------------------------------------------------------------
def _fixed(w_int, b_int, ws_int, bs_int, q_w, q_b, minus_four, n_inter, residual):
    shift_b = 2 * WEIGHT_SHIFT + q_b
    assert shift_b >= 0
    w, b = [], []
    for l, (wl, bl) in enumerate(zip(w_int, b_int)):
        n_out, n_in = wl.shape
        m = np.empty((n_in, n_out), dtype=object)
        for o in range(n_out):
            for i in range(n_in):
                inter = n_inter > 0 and l == 0 and i >= n_in - n_inter
                shift = WEIGHT_SHIFT + q_w - (FRAC_INTER if inter else 0)
                assert shift >= 0
                v = wrap64(wl[o, i] << shift)
                if residual and n_in == n_out and o == i:
                    v = wrap64(v + (1 << (WEIGHT_SHIFT - (FRAC_INTER if inter else 0))))
                m[i, o] = v
        bias = [int(v) for v in bl]
        if minus_four and l == len(w_int) - 1:
            bias[1] = wrap64(bias[1] - (4 << -q_b))
        w.append(m)
        b.append(np.array([wrap64(v << shift_b) for v in bias], dtype=object))
    dim, n_last = w_int[0].shape[1], w_int[-1].shape[0]
    ws = np.zeros((dim, n_last), dtype=object)
    bs = np.zeros(n_last, dtype=object)
    ws[...] = 0
    bs[...] = 0
    if ws_int is not None:
        for o in range(n_last):
            for i in range(dim):
                shift = WEIGHT_SHIFT + q_w - (FRAC_INTER if (n_inter > 0 and i >= dim - n_inter) else 0)
                assert shift >= 0
                ws[i, o] = wrap64(ws_int[o, i] << shift)
            bs[o] = wrap64(bs_int[o] << shift_b)
    return Fixed(w, b, ws, bs)


def fixed_point(arch, ints):
    p = split(arch, ints)
    q = [int(v) for v in arch.nn_q_step_log2]
    arm = _fixed(p["w"], p["b"], p["ws"], p["bs"], q[0], q[1], True, arch.output_feature_ifce, True)
    ifce = [None if w is None else _fixed([w], [b], None, None, q[2], q[3], False, 0, False) for w, b in zip(p["ifce_w"], p["ifce_b"])]
    return Params(arm, ifce)


# ---- forward ---------------------------------------------------------------------------------------------------------
class _Count:
    def __init__(self):
        self.n_wrapped = self.n_sums = 0
        self.max_act = self.max_feat = 0


def _affine(x, w, b, count, wrap=True, extra=None):
    """b + x @ w (+ extra) for x [n][in], w [in][out] in unbounded integers; each of the n * out sums reduced to signed 64 bits
    once (wrap=False: not at all).  Object arrays in and out."""
    n = x.shape[0]
    out = np.empty((n, w.shape[1]), dtype=object)
    xa, wa, ba = np.abs(x.astype(np.float64)), np.abs(w.astype(np.float64)), np.abs(b.astype(np.float64))
    worst = (xa @ wa + ba).max(axis=1) if n else np.zeros(0)
    if extra is not None:
        worst = worst + np.abs(extra.astype(np.float64)).max(axis=1)
    small = worst < 2.0 ** 61  # margin of 2 for the float64 rounding of the bound itself
    if n:
        small &= xa.max(axis=1) < 2.0 ** 62  # (an unreduced input beyond int64 that only meets zero weights)
    if small.any() and max(abs(v) for v in w.ravel()) < 1 << 62:
        y = x[small].astype(np.int64) @ w.astype(np.int64) + b.astype(np.int64)
        if extra is not None:
            y = y + extra[small].astype(np.int64)
        out[small] = _obj(y)
    else:
        small[:] = False
    big = ~small
    if big.any():
        y = np.dot(x[big], w) + b
        if extra is not None:
            y = y + extra[big]
        flat = y.ravel()
        count.n_wrapped += sum(1 for v in flat if not -(1 << 63) <= v < (1 << 63))
        out[big] = _wrap_array(y) if wrap else y
    count.n_sums += out.size
    return out


def _shift(a, s):
    return np.vectorize(lambda v: int(v) >> s, otypes=[object])(a) if a.size else a


def _arm_forward(arm, ctx, count, wrap=True, act=None):
    """ctx [n][dim] raw contexts -> ([n][2] output sums >> 24, [n] largest hidden activation of the pixel)."""
    peak = np.zeros(ctx.shape[0], dtype=object)
    peak[...] = 0
    x = np.vectorize(lambda v: int(v) << WEIGHT_SHIFT, otypes=[object])(ctx)
    stab = _affine(x, arm.ws, arm.bs, count, wrap)
    for w, b in zip(arm.w[:-1], arm.b[:-1]):
        a = _affine(x, w, b, count, wrap)
        x = _shift(np.vectorize(lambda v: v if v > 0 else 0, otypes=[object])(a), 16)
        if act is not None:
            x = np.vectorize(act, otypes=[object])(x)
        if x.size:
            peak = np.maximum(peak, x.max(axis=1))
            count.max_act = max(count.max_act, max(x.ravel()))
    out = _affine(x, arm.w[-1], arm.b[-1], count, wrap, extra=stab)
    return _shift(out, 2 * WEIGHT_SHIFT - FRAC_INTER), peak


def _clip(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def _float32_round_trip(v):
    return int(np.float32(v))  # coolchic.py:142-144; |v| < 2^40 here, exact in the float64 numpy converts through


def context_offsets(n_spatial):
    """[(rows above, signed column offset)] of the n highest-priority causal neighbours."""
    out = [None] * n_spatial
    for pos, rank in enumerate(PRIORITY):
        if rank < n_spatial:
            out[rank] = (4 - pos // 9, pos % 9 - 4)
    return out


def decode_order(h, w):
    """Pixel (y, x) pairs in the order the reference decodes them: raster when w <= 9, else by wavefront x + 10 y (latent.py:240-265)."""
    if w <= 9:
        return [(y, x) for y in range(h) for x in range(w)]
    return sorted(((y, x) for y in range(h) for x in range(w)), key=lambda p: (p[1] + 10 * p[0], p[0]))


def forward(arch, ints, latents, wrap=True, damage=None):
    """Every pixel's (mu_idx, scale_idx) as idx[g] [h][w][2], every grid's IFCE features as features[g] [n_if][h][w] (object; None
    without IFCE), the number of pixels that read a wide feature (|f| >= 2^15 or f = -2^15: ccd_entropy_pipe.hip's rule for the
    int16 plane at its default limit), every pixel's largest hidden activation as peaks[g] [h][w] (object; above 0x7F7F7F: what
    the matrix-core path redoes), and the census.  wrap=False: no sum is ever reduced (what unbounded integers would give).
    damage = {"weight" | "activation" | "feature": f} passes every ARM weight / hidden activation / feature the ARM reads through
    f first - what an evaluation too narrow for the value would compute (tests measure how many table indices that moves: a
    case must be able to tell)."""
    p = fixed_point(arch, ints)
    damage = damage or {}
    if "weight" in damage:
        p = Params(Fixed([np.vectorize(damage["weight"], otypes=[object])(m) for m in p.arm.w], p.arm.b,
                         np.vectorize(damage["weight"], otypes=[object])(p.arm.ws), p.arm.bs), p.ifce)
    n, n_sp, n_if, dim = arch.n_grids, arch.spatial_context_arm, arch.output_feature_ifce, arch.total_context_arm
    has_ifce = bool(arch.has_ifce_resolution) and n_if > 0
    fin = [int(arch.input_features_ifce[g]) for g in range(n)]
    hw = [(int(arch.grid_h[g]), int(arch.grid_w[g])) for g in range(n)]
    offs = context_offsets(n_sp)
    count = _Count()
    idx, feats, wide_pixels, peaks = [None] * n, [None] * n, 0, [None] * n
    for g in range(n - 1, -1, -1):
        h, w = hw[g]
        feat = None
        if has_ifce:
            feat = np.zeros((n_if, h, w), dtype=object)
            feat[...] = 0
        raw = None
        if has_ifce and fin[g] > 0:
            if g == n - 1:
                sh, sw = h, w
                stack = np.zeros((sh * sw, 1), dtype=object)
                stack[...] = 0
            else:
                assert fin[g] == n - 1 - g
                sh, sw = hw[g + 1]
                yy, xx = np.mgrid[0:sh, 0:sw]
                cols, s = [], 0
                for m in range(g + 1, n):
                    if m > g + 1 and hw[m] != hw[m - 1]:
                        s += 1  # one nearest x2 + crop per change of size on the way (upsampling.py:582-588)
                    cols.append(np.asarray(latents[m]).astype(np.int64)[yy >> s, xx >> s].ravel())
                stack = _obj(np.stack(cols, axis=1))
            x = np.vectorize(lambda v: int(v) << WEIGHT_SHIFT, otypes=[object])(stack)
            f = p.ifce[g]
            out = _shift(_affine(x, f.w[0], f.b[0], count, wrap), 2 * WEIGHT_SHIFT - FRAC_INTER)  # [sh * sw][n_if]
            raw = out.reshape(sh, sw, n_if)
            yy, xx = np.mgrid[0:h, 0:w]
            for k in range(n_if):  # nearest x2 and crop (coolchic.py:142-146), through float32 and back
                plane = np.vectorize(_float32_round_trip, otypes=[object])(raw[:, :, k])
                feat[k] = plane[yy >> 1, xx >> 1]
            count.max_feat = max(count.max_feat, max(abs(v) for v in raw.ravel()))
            widef = np.vectorize(lambda v: v >= 1 << 15 or v <= -(1 << 15), otypes=[bool])(raw).any(axis=2)
            wide_pixels += int(widef[yy >> 1, xx >> 1].sum())
        feats[g] = feat
        lat = np.zeros((h + 4, w + 8), dtype=np.int64)
        lat[4:, 4:w + 4] = np.asarray(latents[g]).astype(np.int64)
        ctx = np.empty((h * w, dim), dtype=object)
        for k, (dy, dx) in enumerate(offs):
            ctx[:, k] = _obj(lat[4 - dy:4 - dy + h, 4 + dx:4 + dx + w].ravel())
        for k in range(dim - n_sp):
            ctx[:, n_sp + k] = feat[k].ravel() if feat is not None else 0
            if "feature" in damage:
                ctx[:, n_sp + k] = np.vectorize(damage["feature"], otypes=[object])(ctx[:, n_sp + k])
        ms, peak = _arm_forward(p.arm, ctx, count, wrap, damage.get("activation"))
        peaks[g] = peak.reshape(h, w)
        grid = np.empty((h * w, 2), dtype=np.int64)
        for i in range(h * w):
            grid[i, 0] = _clip(_clip(ms[i, 0], -1000000, 1000000) + MU_OFFSET, 0, N_MU - 1)
            grid[i, 1] = _clip(_clip(ms[i, 1], -1000000, 1000000) + SCALE_OFFSET, 0, N_SCALE - 1)
        idx[g] = grid.reshape(h, w, 2)
    max_w = max([abs(v) for m in p.arm.w for v in m.ravel()] + [abs(v) for v in p.arm.ws.ravel()])
    return Forward(idx, feats, wide_pixels, peaks, Census(max_w, count.max_act, count.max_feat, count.n_wrapped, count.n_sums))


def in_decode_order(idx_g):
    h, w, _ = idx_g.shape
    return np.array([idx_g[y, x] for y, x in decode_order(h, w)], dtype=np.int64).reshape(-1, 2)


# ---- classification --------------------------------------------------------------------------------------------------
def _bounds(fx, in_bound, shift):
    """Worst-case magnitudes through a fixed-point MLP for |input i| <= in_bound[i]: (32-bit operands and sums below 2^62
    guaranteed?, output bound, hidden bounds per layer)."""
    ok = True
    x = [v << 16 for v in in_bound]
    ok &= all(v <= LIM32 for v in x)
    stab = []
    for o in range(fx.ws.shape[1]):
        acc = abs(fx.bs[o]) + sum(xi * abs(fx.ws[i, o]) for i, xi in enumerate(x))
        ok &= all(abs(v) <= LIM32 for v in fx.ws[:, o]) and acc < 1 << 62
        stab.append(acc)
    hidden = []
    for l, (w, b) in enumerate(zip(fx.w, fx.b)):
        last = l == len(fx.w) - 1
        y = []
        for o in range(w.shape[1]):
            acc = abs(b[o]) + sum(xi * abs(w[i, o]) for i, xi in enumerate(x)) + (stab[o] if last else 0)
            ok &= all(abs(v) <= LIM32 for v in w[:, o]) and acc < 1 << 62
            y.append((acc >> (shift if last else 16)) + 1)
            if not last:
                ok &= y[-1] <= LIM32
        if not last:
            hidden.append(max(y))
        x = y
    return ok, max(x), hidden


def classify(arch, ints):
    """The decisions of ccd_format.cpp::decode_network, ccd_batch_plan.cpp::choose_entropy_kernel and entropy_pipe_supports[_mfma]
    for a network, from its integers.  (The library clamps intermediate bounds at 2^40 / 2^62 to stay inside 128 bits; a clamped
    bound times a non-zero weight is still beyond int32 after >> 16, so the clamps change no decision and are not restated.)
    mfma / pipe hold for pictures whose grids fit the symbol ring and whose tables fit the LDS (every case here)."""
    p = fixed_point(arch, ints)
    dim, n_sp, n_if = arch.total_context_arm, arch.spatial_context_arm, arch.output_feature_ifce
    n_layers = arch.n_hidden_layers_arm + 1
    worst_feature = 0
    for g in range(arch.n_grids):
        if p.ifce[g] is not None:
            worst_feature = max(worst_feature, _bounds(p.ifce[g], [64] * int(arch.input_features_ifce[g]), 24)[1])
    in_bound = [64] * n_sp + [worst_feature] * (dim - n_sp)
    ok, _, hidden = _bounds(p.arm, in_bound, 24)
    narrow = ok and worst_feature < 1 << 24
    arm_w = [abs(v) for m in p.arm.w for v in m.ravel()] + [abs(v) for v in p.arm.ws.ravel()]
    w32 = all(v <= LIM32 for v in arm_w)
    ifce_w32 = all(abs(v) <= LIM32 for f in p.ifce if f is not None for v in f.w[0].ravel())
    dyn_act = (not w32) or any(v > LIM32 for v in hidden)
    feat_i32 = worst_feature < 1 << 30
    dyn_feat = worst_feature >= 1 << 15
    pipe = w32 and feat_i32 and not dyn_act and dim <= 32 and n_layers <= 8
    # a feature lies in [-bound, bound - 1]: two signed digits hold it iff bound - 1 <= 0x7F7F
    mfma = (pipe and narrow and dim <= 20 and 2 <= n_layers <= 8 and n_if <= 8 and max(arm_w) <= DIGITS3_MAX
            and worst_feature <= DIGITS2_MAX + 1)
    return Flags(w32, dyn_act, dyn_feat, feat_i32, ifce_w32, narrow, max(arm_w), worst_feature, mfma, pipe)


def signed_digits(v, n):
    """The n signed-digit bytes the matrix-core path splits an operand into (mf_byte / mf_pack15 restated): the bytes of
    (v + 0x80..80) ^ 0x80..80 read as int8, lowest first."""
    k = int("80" * n, 16)
    d = ((v + k) & 0xFFFFFFFF) ^ k
    return [((d >> (8 * j)) & 0xFF) - (((d >> (8 * j)) & 0x80) << 1) for j in range(n)]


def keep_digits(n):
    """v -> what n signed-digit bytes keep of it."""
    return lambda v: sum(d << (8 * j) for j, d in enumerate(signed_digits(int(v), n)))


def keep_bits(n):
    """v -> v reduced to a signed n-bit integer."""
    return lambda v: ((int(v) + (1 << (n - 1))) & ((1 << n) - 1)) - (1 << (n - 1))
