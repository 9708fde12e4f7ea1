"""A float64 statement of the whole float path for ANY header the decoder accepts, written from the operations the reference
decoder calls (upsampling.py: conv_transpose2d behind a replicate pad, the kron pre-concatenation conv2d; synthesis.py: conv2d
behind F.pad(mode="replicate"), residual, ReLU, stabiliser, output transform), not from the loops of oracle/cc_oracle.c, whose
tconv_up2 / preconv / syn_conv share their structure with the device's generic kernels and are pinned to the reference only at the
fixtures' kernel sizes (tests/test_synth_arch.py).

Parameters: writer.dequantise_network of the stream's own integers.  ups.w holds n_ups x ceil(k / 2) halves of the transposed
convolution's symmetric filters, then n_ups x ceil(k_pre / 2) of the pre-concatenation filters; step s of the pyramid (coarsest
first) takes filter s mod n_ups.  syn.w and syn.b hold output transform, stabiliser, layers.

The bar of a float32 evaluation `got` of a stage against its float64 value `ref64` (the rule of tests/float_tail_ref.py):

    |got - ref64| <= 2 * max|torch float32 run of the same chain - ref64| + FLOOR_ULPS * 2^-23 * max|ref64|

the measured term is what float32 costs on this very network and input, the factor 2 allows another evaluation order to land on
the other side of the float64 value, and the floor of 8 units of 2^-23 max|ref64| covers the stages where the measured term is
rounding noise alone: the float32 products of two filter taps, the multiply-adds of a tap chain and the sums of the residual,
stabiliser and output transform are some 8 roundings of relative size 2^-24 on the way to an output.  A wrong tap, crop, clamp
or filter index gives errors of 1e-2 max|ref64| and more."""
import numpy as np

FLOOR_ULPS = 8.0


def parameters(arch, nn_bytes):
    """{"ups": [n_ups][k], "pre": [n_ups][k_pre] symmetric 1-D filters, "out": (w, b), "stab": (w, b) | None,
    "layers": [(w [c_out][c_in][k][k], b, residual, relu)]} as float32 arrays."""
    from cool_chic_amd import writer

    values = writer.dequantise_network(arch, writer.network_values(arch, nn_bytes))
    groups = np.split(values, np.cumsum(writer.network_layout(arch))[:-1])
    n_ups, k, kp = arch.latent_resolution[1], arch.ups_k_size, arch.ups_preconcat_k_size

    def symmetric(p, size):
        p = list(p)
        return np.array(p + p[::-1][size % 2:], np.float32)

    nu, npre = (k + 1) // 2, (kp + 1) // 2
    ups = [symmetric(groups[4][i * nu:(i + 1) * nu], k) for i in range(n_ups)]
    pre = [symmetric(groups[4][n_ups * nu + i * npre:n_ups * nu + (i + 1) * npre], kp) for i in range(n_ups)]
    assert all(u.size == k for u in ups) and all(p.size == kp for p in pre)
    c, ci = arch.out_channels, arch.input_feature_synthesis
    n_stab = ci // 2 if arch.flag_common_randomness else ci
    w, b, pw, pb = groups[6], groups[7], 0, 0

    def take(c_out, c_in, ks):
        nonlocal pw
        a = w[pw:pw + c_out * c_in * ks * ks].reshape(c_out, c_in, ks, ks)
        pw += a.size
        return a

    def take_b(n):
        nonlocal pb
        a = b[pb:pb + n]
        pb += n
        return a

    out_w = take(c, c, 1)
    stab_w = take(c, n_stab, 1) if arch.linear_stabiliser_synth else None
    layer_w, c_in = [], ci
    for l in range(arch.n_layer_synthesis):
        s = arch.syn_layer[l]
        layer_w.append(take(s.out_ft, c_in, s.k_size))
        c_in = s.out_ft
    out_b = take_b(c)
    stab_b = take_b(c) if arch.linear_stabiliser_synth else None
    layers = [(layer_w[l], take_b(arch.syn_layer[l].out_ft), arch.syn_layer[l].mode == 1, arch.syn_layer[l].non_linearity == 1)
              for l in range(arch.n_layer_synthesis)]
    assert pw == w.size and pb == b.size
    return {"ups": ups, "pre": pre, "out": (out_w, out_b), "stab": None if stab_w is None else (stab_w, stab_b), "layers": layers}


def pyramid(par, latents, dtype):
    """Upsampling.forward: `latents` = the non-hyper grids, finest first -> [levels][h][w] (channel 0 = the finest level)."""
    import torch
    import torch.nn.functional as F

    x = torch.from_numpy(np.ascontiguousarray(latents[-1])).to(dtype)[None, None]
    for step, target in enumerate(reversed(latents[:-1])):
        u = torch.from_numpy(par["ups"][step % len(par["ups"])]).to(dtype)
        p = torch.from_numpy(par["pre"][step % len(par["pre"])]).to(dtype)
        k, kp = u.numel(), p.numel()
        t = torch.from_numpy(np.ascontiguousarray(target)).to(dtype)[None, None]
        p0 = k // 2
        crop = 2 * p0 - 1 + k // 2
        xp = F.pad(x.transpose(0, 1), (p0, p0, p0, p0), mode="replicate")   # every channel on its own: [c][1][h][w]
        y = F.conv_transpose2d(xp, torch.outer(u, u)[None, None], stride=2)
        y = y[:, :, crop:y.shape[2] - crop, crop:y.shape[3] - crop][:, :, :t.shape[2], :t.shape[3]]
        assert y.shape[2:] == t.shape[2:], (y.shape, t.shape)
        t = F.conv2d(t, torch.outer(p, p)[None, None], padding=kp // 2) + t
        x = torch.cat((t, y.transpose(0, 1)), dim=1)
    return x[0]


def synthesis(par, dense, dtype):
    """Synthesis.forward on the dense stack [c_in][h][w]: main branch + stabiliser of the latent channels, output transform."""
    import torch
    import torch.nn.functional as F

    def T(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)

    x0 = dense[None]
    x = x0
    for w, b, residual, relu in par["layers"]:
        pad = (w.shape[2] - 1) // 2
        y = F.conv2d(F.pad(x, (pad, pad, pad, pad), mode="replicate"), T(w), T(b))
        if residual:
            y = y + x
        x = torch.relu(y) if relu else y
    if par["stab"] is not None:
        w, b = par["stab"]
        x = x + F.conv2d(x0[:, :w.shape[1]], T(w), T(b))
    w, b = par["out"]
    return F.conv2d(x, T(w), T(b))[0]


def float_path(arch, nn_bytes, latents, noise=None):
    """{stage: (ref64, torch float32 run)} for the stages "dense" (the latent channels of the dense stack) and "syn_out" (the
    synthesis output before any final resize).  `latents`: every grid of the stream in stream order; `noise`: the noise channels of
    a common-randomness stream's dense stack (given: they are pinned by tests/test_float_tail.py), appended behind the pyramid."""
    import torch

    par = parameters(arch, nn_bytes)
    lat = [latents[g] for g in range(arch.n_grids) if not arch.is_hyperlatent[g]]
    out = {"dense": [], "syn_out": []}
    for dtype in (torch.float64, torch.float32):
        dense = pyramid(par, lat, dtype)
        out["dense"].append(dense.numpy())
        if noise is not None:
            dense = torch.cat((dense, torch.from_numpy(np.ascontiguousarray(noise)).to(dtype)), dim=0)
        out["syn_out"].append(synthesis(par, dense, dtype).numpy())
    return {k: (v[0], v[1]) for k, v in out.items()}


def bar(ref64, run32):
    """(bar, measured) of the module docstring."""
    measured = float(np.abs(run32.astype(np.float64) - ref64).max())
    return 2.0 * measured + FLOOR_ULPS * 2.0 ** -23 * float(np.abs(ref64).max()), measured
